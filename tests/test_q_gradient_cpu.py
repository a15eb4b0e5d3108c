"""q_gradient() without a GPU: the two-head packers are adjoint and agree with pack_mlp on the shared part; the fp64
restatement the GPU tests hold the kernels to (tests/q_restatement.py) is the gradient of the TD loss by torch autograd
with the target detached; it tells wrong estimators apart; every case of the GPU file, replayed by the NumPy oracle,
keeps its ambiguity shares under the cap and is not trivial; and every refusal comes before the library is touched
(the Python checks) or before the handle is read (the C entry point, in the order of its body)."""
import ctypes as C
import itertools
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q_gradient_cases as QC  # noqa: E402
from q_restatement import AMBIGUOUS_CAP, q_fp64  # noqa: E402

from weather2alert_amd import _ffi, build, policy  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_OBS = 20
OBS_SLOT = [2 + j for j in range(N_OBS)]  # an injective map into slots 0..29 that is not the identity
# the shapes q_gradient() was specified with, which reach five <WIDTH, LAYERS> pairs ((24, 40) pads to <64, 2>), and
# (24, 20) for <32, 2>: all six pairs, padded units in six of the seven nets
SHAPES = [(7,), (24,), (40,), (7, 13), (24, 20), (24, 40), (64, 64)]


def _net(rng, hidden, G_=3, n_obs=N_OBS, scale=1.0):
    dims = [n_obs] + list(hidden) + [2]
    return [((rng.standard_normal((G_, dims[i + 1], dims[i])) * scale / np.sqrt(dims[i])).astype(np.float32),
             (rng.standard_normal((G_, dims[i + 1])) * 0.5).astype(np.float32)) for i in range(len(dims) - 1)]


@pytest.mark.parametrize("hidden", SHAPES)
def test_pack_and_unpack_are_adjoint_and_share_pack_mlp_s_front(hidden):
    """<pack(L), P> = <L, unpack(P)> on the seven shapes (all six <WIDTH, LAYERS> pairs); the first mlp_stride - 4 floats
    are pack_mlp's of the one-output net made of the same hidden layers and row 0; the second row and both biases sit where w2a.h says"""
    rng = np.random.default_rng(len(hidden) * 100 + hidden[0])
    L = _net(rng, hidden)
    P, w, nl, G_ = policy.pack_mlp_heads(L, OBS_SLOT, N_OBS)
    assert (w, nl, G_) == (policy.mlp_width(hidden), len(hidden), 3)
    st = policy.mlp_stride(w, nl)
    assert tuple(P.shape) == (3, policy.mlp_heads_stride(w, nl)) and policy.mlp_heads_stride(w, nl) == st + w
    assert P.dtype == torch.float32 and policy.mlp_heads_stride(w, nl) % 4 == 0  # rows stay 16-B aligned
    one = lambda a: L[:-1] + [(L[-1][0][:, a:a + 1], L[-1][1][:, a:a + 1])]  # noqa: E731
    P0, P1 = policy.pack_mlp(one(0), OBS_SLOT, N_OBS)[0], policy.pack_mlp(one(1), OBS_SLOT, N_OBS)[0]
    assert torch.equal(P[:, :st - 4], P0[:, :st - 4])
    assert torch.equal(P[:, st - 4:st - 4 + w], P1[:, st - 4 - w:st - 4])
    assert torch.equal(P[:, st - 4 + w], P0[:, st - 4]) and torch.equal(P[:, st - 3 + w], P1[:, st - 4])
    assert bool((P[:, st - 2 + w:] == 0).all())
    R = torch.as_tensor(rng.standard_normal(tuple(P.shape)))
    back = policy.unpack_mlp_heads_grad(R, OBS_SLOT, N_OBS, hidden)
    assert [(tuple(a.shape), tuple(b.shape)) for a, b in back] == [(W.shape, b.shape) for W, b in L]
    lhs = float((P.double() * R).sum())
    rhs = sum(float((torch.as_tensor(W).double() * dW).sum() + (torch.as_tensor(b).double() * db).sum())
              for (W, b), (dW, db) in zip(L, back))
    assert abs(lhs - rhs) <= 1e-12 * float((P.double().abs() * R.abs()).sum())
    with pytest.raises(ValueError, match="exactly 2 rows"):
        policy.pack_mlp_heads(one(0), OBS_SLOT, N_OBS)
    with pytest.raises(ValueError):
        policy.unpack_mlp_heads_grad(R[:, :-1], OBS_SLOT, N_OBS, hidden)


def test_grad_to_module_writes_the_negated_gradient_on_an_sb3_shaped_q_net():
    q_net = torch.nn.Sequential(torch.nn.Linear(N_OBS, 24), torch.nn.ReLU(), torch.nn.Linear(24, 40), torch.nn.ReLU(),
                                torch.nn.Linear(40, 2))
    pol = policy.mlp_from_module(q_net)
    assert pol["layers"][-1][0].shape[0] == 2
    P = policy.pack_mlp_heads(pol["layers"], OBS_SLOT, N_OBS)[0]
    grad = {"layers": policy.unpack_mlp_heads_grad(torch.arange(P.numel(), dtype=torch.float32).reshape(P.shape), OBS_SLOT,
                                                   N_OBS, (24, 40))}
    policy.mlp_heads_grad_to_module(q_net, grad)
    lins = [m for m in q_net if isinstance(m, torch.nn.Linear)]
    for m, (dW, db) in zip(lins, grad["layers"]):
        assert torch.equal(m.weight.grad, -dW[0]) and torch.equal(m.bias.grad, -db[0])
    one_row = {"layers": grad["layers"][:-1] + [(grad["layers"][-1][0][:, :1], grad["layers"][-1][1][:, :1])]}
    with pytest.raises(ValueError):
        policy.mlp_heads_grad_to_module(q_net, one_row)


# ---- the restatement against autograd ---------------------------------------------------------------------------------
def _toy(seed, n=12, S=10, n_obs=N_OBS):
    """12 envs, 10 days: random rows, rewards and actions; envs that end early, one finished on entry, budgets that
    run out"""
    rng = np.random.default_rng(seed)
    days = rng.integers(3, S + 3, n)  # > S: still running when the call ends
    days[0] = 0
    valid = np.arange(S)[:, None] < days[None, :]
    terminal = valid & (np.arange(S)[:, None] == (days - 1)[None, :])
    return dict(obs=rng.standard_normal((S + 1, n, n_obs)).astype(np.float32).astype(np.float64), valid=valid,
                terminal=terminal, issued=(rng.random((S, n)) < 0.4) & valid, attempted=(rng.random((S, n)) < 0.6) & valid,
                reward=rng.standard_normal((S, n)) * 0.7, left_after=rng.integers(-1, 3, (S, n)),
                g=np.array([0, 1, 3])[np.arange(n) % 3], w=rng.standard_normal(n))


def _autograd(T, layers, target, act, gamma, double, loss, hd, bootstrap, rb, G_=4):
    """-d/dtheta of mean_g-weighted sum_e w_e sum_s l(y_s.detach() - Q(o_s, a_s)) in float64: [(dW, db), ...]"""
    f = torch.tanh if act == "tanh" else torch.relu
    gt = torch.as_tensor(T["g"])

    def heads(P, x):
        h = x
        for W, b in P[:-1]:
            h = f(torch.einsum("snj,nuj->snu", h, W[gt]) + b[gt][None])
        return torch.einsum("snj,nuj->snu", h, P[-1][0][gt]) + P[-1][1][gt][None]

    mk = lambda L: [(torch.tensor(np.asarray(W, np.float64), requires_grad=True),  # noqa: E731
                     torch.tensor(np.asarray(b, np.float64), requires_grad=True)) for W, b in L]
    P = mk(layers)
    Pt = P if target is None else mk(target)
    x = torch.as_tensor(T["obs"])
    valid, term = torch.as_tensor(T["valid"]), torch.as_tensor(T["terminal"])
    S = valid.shape[0]
    Q = heads(P, x)
    with torch.no_grad():
        Qn, Qtn = Q[1:], heads(Pt, x)[1:]
        nxt = torch.where(Qn[..., 1] > Qn[..., 0], Qtn[..., 1], Qtn[..., 0]) if double else Qtn.max(dim=-1).values
        if rb:
            nxt = torch.where(torch.as_tensor(T["left_after"]) <= 0, Qtn[..., 0], nxt)
        has_next = valid & ~term
        if not bootstrap:
            has_next[S - 1] = False
        y = torch.as_tensor(T["reward"]) + gamma * torch.where(has_next, nxt, torch.zeros_like(nxt))
    a = torch.as_tensor(T["issued"]).long()
    delta = y - torch.gather(Q[:S], 2, a[..., None])[..., 0]
    if loss == "huber":
        l = torch.nn.functional.huber_loss(delta, torch.zeros_like(delta), reduction="none", delta=hd)
    else:
        l = 0.5 * delta * delta
    cnt = torch.as_tensor(np.maximum(np.bincount(T["g"], minlength=G_), 1).astype(np.float64))
    total = (torch.as_tensor(T["w"])[None, :] * torch.where(valid, l, torch.zeros_like(l)) / cnt[gt][None, :]).sum()
    (-total).backward()
    return [(W.grad.numpy(), b.grad.numpy()) for W, b in P], l.detach().numpy() * T["valid"]


SETTINGS = [dict(loss=lo, double=d, bootstrap=b, rb=rb, target=t)
            for lo, d, b, rb, t in itertools.product(("huber", "squared"), (False, True), (False, True), (False, True),
                                                     (False, True)) if not (rb and not b and not d)]


@pytest.mark.parametrize("hidden,act", [((7,), "tanh"), ((24, 20), "relu"), ((24, 40), "relu"), ((64, 64), "tanh")])
def test_restatement_is_the_semi_gradient_by_autograd(hidden, act):
    """12 envs, 10 days, to 1e-10: squared and Huber loss, double on and off, bootstrap on and off, require_budget
    masking, the online net as its own target and a distinct one; y detached"""
    rng = np.random.default_rng(5)
    T = _toy(3)
    layers, target = _net(rng, hidden, 4), _net(rng, hidden, 4)
    seen_masked = seen_clamped = False
    for kw in SETTINGS:
        tg = target if kw["target"] else None
        ref = q_fp64(T["obs"], T["issued"], T["valid"], T["terminal"], T["reward"], T["left_after"], T["w"], layers, tg, act,
                     T["g"], 4, gamma=0.9, double=kw["double"], loss=kw["loss"], huber_delta=0.8, bootstrap=kw["bootstrap"],
                     require_budget=kw["rb"])
        want, l = _autograd(T, layers, tg, act, 0.9, kw["double"], kw["loss"], 0.8, kw["bootstrap"], kw["rb"])
        scale = max(np.abs(x).max() for wb in want for x in wb)
        assert scale > 0
        for (dW, db), (aW, ab) in zip(ref["layers"], want):
            have = ~np.isnan(dW).reshape(dW.shape[0], -1).all(axis=1)
            assert list(have) == [True, True, False, True]  # group 2 is empty
            assert np.abs(dW[have] - aW[have]).max() <= 1e-10 * scale and np.abs(db[have] - ab[have]).max() <= 1e-10 * scale, kw
        assert np.abs(ref["loss"] - l.sum(axis=0)).max() <= 1e-10 * max(1.0, np.abs(l).max())
        assert ref["days"][0] == 0 and ref["loss"][0] == 0  # finished on entry
        seen_masked |= bool(ref["masked"].any())
        seen_clamped |= kw["loss"] == "huber" and bool((np.abs(ref["td_error"]) > 0.8).any()) and \
            bool(((np.abs(ref["td_error"]) < 0.8) & T["valid"]).any())
    assert seen_masked and seen_clamped


def _outside(got, ref):
    return any((np.abs(x - r)[~np.isnan(r)] > bd[~np.isnan(r)]).any() for wb, rb, bb in zip(got, ref["layers"], ref["bound"])
               for x, r, bd in zip(wb, rb, bb))


def test_the_restatement_tells_a_wrong_estimator_apart():
    """the head of the ATTEMPTED action instead of the issued one, require_budget's mask ignored, the online net valued as
    its own target, double-DQN's choice dropped, gamma off by 0.01: each leaves the bound of the right one"""
    rng = np.random.default_rng(6)
    T = _toy(4)
    layers, target = _net(rng, (24, 40), 4), _net(rng, (24, 40), 4)
    args = (T["obs"], T["issued"], T["valid"], T["terminal"], T["reward"], T["left_after"], T["w"], layers, target, "tanh",
            T["g"], 4)
    kw = dict(gamma=0.9, double=True, loss="huber", huber_delta=0.8, bootstrap=True, require_budget=True)
    ref = q_fp64(*args, **kw)
    assert not _outside(q_fp64(*args, **kw)["layers"], ref)
    for what, other in (("attempted", dict(kw, mutant="attempted", attempted=T["attempted"])),
                        ("no_mask", dict(kw, mutant="no_mask")), ("online_target", dict(kw, mutant="online_target")),
                        ("max for argmax", dict(kw, double=False)), ("gamma", dict(kw, gamma=0.91))):
        assert _outside(q_fp64(*args, **other)["layers"], ref), what


# ---- the GPU file's cases, replayed by the oracle ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def tabs():
    return QC.make_tables()


def _reference(tabs, name, n=None, gid0=None, group=None, layers=None, target=None):
    c = QC.case(name)
    tb = tabs[c["table"]]
    n = c["n"] if n is None else n
    gid0 = QC.E.GID0 if gid0 is None else gid0
    sched = QC.schedule(tb, c["table"], c, n, gid0)
    R = QC.oracle_rows(tb, c["table"], c, n, sched, gid0)
    if layers is None:
        g = QC.groups(n) if c["grouped"] else None
        layers, target = QC.nets(tb.ct, c, QC.G if c["grouped"] else 1)
    else:
        g = group
    w = QC.weights(n) if c["weights"] else None
    ref = q_fp64(R["obs"], R["issued"], R["valid"], R["terminal"], R["reward"], R["left_after"], w, layers, target, c["act"],
                 g, None if g is None else QC.G, gamma=c["gamma"], double=c["double"], loss=c["loss"],
                 huber_delta=c["huber_delta"], bootstrap=c["bootstrap"], require_budget=c["rb"])
    return c, R, ref


def _not_trivial(c, R, ref, what):
    d = np.abs(ref["td_error"])[R["valid"]]
    assert d.size and (d > 0).any(), what
    if c["loss"] == "huber":
        assert (d > c["huber_delta"]).any() and (d < c["huber_delta"]).any(), (what, float(d.min()), float(d.max()))
    if c["rb"]:
        assert ref["masked"].any() and (ref["has_next"] & ~ref["masked"]).any(), what
    assert R["issued"].any() and (R["valid"] & ~R["issued"]).any(), what  # both heads are scored


@pytest.mark.parametrize("name", list(QC.CASES))
def test_gpu_cases_stay_under_the_ambiguity_cap(tabs, name):
    """near_tie + near_kink <= AMBIGUOUS_CAP from the restatement alone, and the case is not trivial: TD errors on both
    sides of huber_delta, both actions taken, masked and unmasked next rows where require_budget is on"""
    c, R, ref = _reference(tabs, name)
    print(f"{name}: near_tie {ref['near_tie']:.2e}, near_kink {ref['near_kink']:.2e}, |delta| > huber_delta on "
          f"{float((np.abs(ref['td_error'])[R['valid']] > c['huber_delta']).mean()):.2f} of the days, masked "
          f"{int(ref['masked'].sum())} of {int(ref['has_next'].sum())} next rows")
    assert ref["near_tie"] + ref["near_kink"] <= AMBIGUOUS_CAP
    _not_trivial(c, R, ref, name)
    if "ragged" in name:
        assert (~R["valid"][0]).any() and R["valid"][0].any()
    assert QC.INSTANTIATION[c["net"]] == (policy.mlp_width(QC.NETS[c["net"]][0]), len(QC.NETS[c["net"]][0]))


def test_gpu_cases_reach_every_instantiation_under_both_activations():
    """by the host's own padding rule, not by the nets' names: the 1-tile cases run all six <WIDTH, LAYERS> pairs under
    tanh and under ReLU, the 3-tile cases all six pairs and <32, 2> under both"""
    pairs = {(w, nl) for w in policy.MLP_WIDTHS for nl in (1, 2)}
    inst = lambda c: (policy.mlp_width(QC.NETS[c["net"]][0]), len(QC.NETS[c["net"]][0]))  # noqa: E731
    assert {k: inst(dict(net=k)) for k in QC.NETS} == QC.INSTANTIATION
    assert {(7,), (24,), (40,), (7, 13), (24, 40), (64, 64)} <= {h for h, _ in QC.NETS.values()}  # the specified shapes
    small = {(inst(QC.case(n)), QC.case(n)["act"]) for n in QC.CASES}
    assert small == {(p, a) for p in pairs for a in ("tanh", "relu")}
    large = {(inst(QC.case(n)), QC.case(n)["act"]) for n in QC.LARGE}
    assert {p for p, _ in large} == pairs and {((32, 2), "tanh"), ((32, 2), "relu")} <= large
    assert {policy.mlp_width(h) * 4 + len(h) for h in SHAPES} == {w * 4 + nl for w, nl in pairs}


@pytest.mark.parametrize("name", list(QC.LARGE))
def test_large_gpu_cases_stay_under_the_ambiguity_cap(tabs, name):
    """the groups the 3-tiles-per-wave cases check, rebuilt as small batches with the same global env ids"""
    c = QC.case(name)
    ct = tabs[c["table"]].ct
    n_groups = (c["n"] + QC.GROUP_SIZE - 1) // QC.GROUP_SIZE
    online, target = QC.nets(ct, c, 1)
    online, target = QC.scaled(online, n_groups, 10), (None if target is None else QC.scaled(target, n_groups, 11))
    for k in QC.CHECKED:
        nk = min(QC.GROUP_SIZE, c["n"] - k * QC.GROUP_SIZE)
        pick = lambda L: None if L is None else [(W[k:k + 1], b[k:k + 1]) for W, b in L]  # noqa: E731
        _, R, ref = _reference(tabs, name, n=nk, gid0=QC.E.GID0 + k * QC.GROUP_SIZE, layers=pick(online), target=pick(target))
        assert ref["near_tie"] + ref["near_kink"] <= AMBIGUOUS_CAP, (name, k, ref["near_tie"], ref["near_kink"])
        _not_trivial(c, R, ref, (name, k))


# ---- refusals before the library is touched ---------------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the arguments were refused")


def _fake_env(tabs, reward_mode="sampled", fixes=()):
    from weather2alert_amd import HeatAlertVecEnv

    ct = tabs["short"].ct
    env = types.SimpleNamespace(ct=ct, num_envs=6, device=torch.device("cpu"), fixes=tuple(fixes), reward_mode=reward_mode,
                                _needs_reset=True, _obs_current=True, _lib=_NoLibrary(), _h=None)
    return env, ct, (lambda *a, **k: HeatAlertVecEnv.q_gradient(env, *a, **k))


def test_every_refusal_comes_before_the_library(tabs):
    env, ct, call = _fake_env(tabs)
    n, rng = env.num_envs, np.random.default_rng(1)
    q = dict(kind="mlp", layers=_net(rng, (7, 13), 1, ct.n_obs), activation="tanh")
    tg = dict(kind="mlp", layers=_net(rng, (7, 13), 1, ct.n_obs), activation="tanh")
    sched = np.zeros((n, ct.T), bool)
    with pytest.raises(RuntimeError, match="reset"):  # every argument is fine: the call gets as far as the state
        call(q, sched, target_net=tg, double=True, td_error=True, td_target=True, bootstrap=True, n_steps=3,
             env_weight=np.ones(n, np.float32))
    one_row = dict(q, layers=q["layers"][:-1] + [(q["layers"][-1][0][:, :1], q["layers"][-1][1][:, :1])])
    grouped = dict(q, layers=_net(rng, (7, 13), 2, ct.n_obs), group=np.arange(n) % 2)
    bad_q = [one_row, dict(q, allowed_days=np.ones((n, ct.T), bool)), dict(q, sample=True),
             dict(grouped, order=np.arange(n)[::-1].copy()), dict(q, kind="linear"), None, dict(q, activation="gelu")]
    for bad in bad_q:
        with pytest.raises(ValueError):
            call(bad, sched)
    call_ok = lambda **k: call(q, sched, **k)  # noqa: E731
    bad_target = [dict(tg, layers=_net(rng, (7, 12), 1, ct.n_obs)), dict(tg, layers=_net(rng, (7,), 1, ct.n_obs)),
                  dict(tg, activation="relu"), dict(tg, layers=_net(rng, (7, 13), 2, ct.n_obs)), dict(tg, kind="linear"),
                  dict(tg, layers=one_row["layers"]), "q"]
    for bad in bad_target:
        with pytest.raises(ValueError):
            call_ok(target_net=bad)
    for kw in (dict(gamma=1.5), dict(gamma=float("nan")), dict(gamma=True), dict(double=1), dict(loss="l1"),
               dict(huber_delta=0.0), dict(huber_delta=float("inf")), dict(bootstrap=1), dict(td_error=1),
               dict(td_target="yes"), dict(n_steps=0), dict(n_steps=2.5), dict(env_weight=np.ones(n + 1, np.float32)),
               dict(env_weight=np.full(n, np.nan, np.float32)), dict(env_weight=np.ones(n, np.int64))):
        with pytest.raises(ValueError):
            call_ok(**kw)
    for bad_sched in (None, sched[:, :-1], sched.astype(np.int32), sched[:-1]):
        with pytest.raises(ValueError):
            call(q, bad_sched)
    # where value_gradient() refuses because rewards enter
    for kw in (dict(reward_mode="posterior_mean"), dict(fixes=("lag",))):
        _, _, other = _fake_env(tabs, **kw)
        with pytest.raises(ValueError):
            other(q, sched)
    # a group-major "order" and a one-group net with any order are taken
    with pytest.raises(RuntimeError, match="reset"):
        call(dict(grouped, order=policy.group_order(torch.as_tensor(np.arange(n) % 2))), sched)
    with pytest.raises(RuntimeError, match="reset"):
        call(dict(q, order=np.arange(n)[::-1].copy(), require_budget=True), sched)


# ---- the C entry point without a handle ---------------------------------------------------------------------------------
P = 4096  # a non-NULL, 256-B aligned address that is never read
NAN, INF = float("nan"), float("inf")
NAMES = ("alert_mask", "mask_words", "env_weight", "n_steps", "obs", "grad", "loss_out", "days", "ret", "gamma", "double_q",
         "loss", "huber_delta", "bootstrap", "td_error", "td_target", "workspace", "workspace_bytes", "stream")
OK = dict(alert_mask=P, mask_words=0, env_weight=None, n_steps=3, obs=P, grad=P, loss_out=P, days=P, ret=P, gamma=0.99,
          double_q=1, loss=1, huber_delta=1.0, bootstrap=0, td_error=None, td_target=None, workspace=P,
          workspace_bytes=1 << 20, stream=None)
CHECKS = [({"q": None}, "NULL q (the online Q-net)"), ({"n_steps": 0}, "n_steps must be positive"), ({"p.params": None}, "NULL params"),
          ({"p.n_groups": -1}, "n_groups must be positive"), ({"p.n_layers": 3}, "n_layers must be 1 or 2"),
          ({"p.width": 48}, "width must be 16, 32 or 64"),
          ({"p.activation": 2}, "activation must be W2A_MLP_TANH or W2A_MLP_RELU"),
          ({"p.params": P + 16 + 8}, "params must be 16-B aligned"),
          ({"alert_mask": None}, "NULL alert_mask (the schedule to follow)"),
          ({"obs": None}, "NULL obs (the rows the agent holds are the first day's input)"),
          ({"grad": None}, "NULL grad, loss, days or ret"), ({"days": None}, "NULL grad, loss, days or ret"),
          ({"p.require_budget": 2}, "require_budget must be 0 or 1"),
          ({"t.params": None}, "NULL params of the target net"),
          ({"t.params": P + 8}, "the target net's params must be 16-B aligned"),
          ({"t.width": 32}, "the target net must have the online net's width, n_layers, activation and n_groups"),
          ({"t.n_groups": 2}, "the target net must have the online net's width, n_layers, activation and n_groups"),
          ({"gamma": 1.5}, "gamma must lie in [0, 1]"), ({"gamma": NAN}, "gamma must lie in [0, 1]"),
          ({"double_q": 2}, "double_q must be 0 or 1"), ({"loss": 2}, "loss must be W2A_Q_LOSS_SQUARED or W2A_Q_LOSS_HUBER"),
          ({"huber_delta": 0.0}, "huber_delta must be finite and positive"),
          ({"huber_delta": INF}, "huber_delta must be finite and positive"), ({"bootstrap": 2}, "bootstrap must be 0 or 1"),
          ({"workspace": None}, "NULL workspace"), ({"workspace": P + 64}, "workspace must be 256-B aligned")]


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


def _call(lib, bad):
    mk = lambda: _ffi.MlpPolicy(params=P, group=None, order=None, n_groups=1, n_layers=2, width=64, activation=0,  # noqa: E731
                                sample=0, require_budget=0, seed=0)
    q, t = mk(), mk()
    a = dict(OK, q=C.byref(q), t=C.byref(t))
    for k, v in bad.items():
        if k.startswith("p."):
            setattr(q, k[2:], v)
        elif k.startswith("t."):
            setattr(t, k[2:], v)
        else:
            a[k] = v
    rc = lib.w2a_q_gradient_mlp(None, a["q"], a["t"], *(a[k] for k in NAMES))
    return rc, lib.w2a_last_error().decode()


def test_c_refusals_without_a_handle_and_their_order(lib):
    """return code and full text of every check that comes before the handle is read; with two bad arguments the earlier
    check reports; a NULL target net is the online net and a squared loss ignores huber_delta"""
    name = "w2a_q_gradient_mlp"
    assert len(NAMES) + 3 == len(lib.w2a_q_gradient_mlp.argtypes)
    assert _call(lib, {}) == (-1, f"{name}: NULL handle")
    assert _call(lib, {"t": None}) == (-1, f"{name}: NULL handle")
    assert _call(lib, {"loss": 0, "huber_delta": NAN}) == (-1, f"{name}: NULL handle")
    for bad, text in CHECKS:
        assert _call(lib, bad) == (-1, f"{name}: {text}"), bad
    pairs = 0
    for (bad1, text1), (bad2, _) in itertools.combinations(CHECKS, 2):
        if bad1.keys() & bad2.keys() or "q" in bad1:
            continue
        assert _call(lib, {**bad2, **bad1}) == (-1, f"{name}: {text1}"), (bad1, bad2)
        pairs += 1
    assert pairs > len(CHECKS)


def test_workspace_size_is_the_value_gradient_layout_at_the_two_head_stride(lib):
    size, base = lib.w2a_q_gradient_mlp_workspace_bytes, lib.w2a_value_gradient_mlp_workspace_bytes
    a256 = lambda v: (v + 255) // 256 * 256  # noqa: E731
    for n, S, G_, w, nl in ((100, 10, 1, 16, 1), (70_000, 153, 5, 64, 2), (1, 1, 3, 32, 2), (300, 153, 4, 64, 1)):
        n_tiles = (n + 63) // 64
        tiles = min(16, max(1, (n_tiles + 1023) // 1024))
        capacity = (n_tiles + tiles - 1) // tiles + min(G_, n)
        st = policy.mlp_stride(w, nl)
        assert size(n, S, G_, w, nl) == base(n, S, G_, w, nl) - a256(8 * capacity * st) + a256(8 * capacity * (st + w))
    for shape in ((0, 10, 1, 16, 1), (100, 0, 1, 16, 1), (100, 10, 0, 16, 1), (100, 10, 1, 48, 1), (100, 10, 1, 16, 3)):
        assert size(*shape) == 0


def test_abi_header_and_ffi_agree_on_the_new_names(lib):
    new = ["w2a_q_gradient_mlp", "w2a_q_gradient_mlp_workspace_bytes"]
    header = open(os.path.join(ROOT, "include", "w2a.h")).read()
    assert set(re.findall(r"\b(w2a_q_gradient_\w+)\s*\(", header)) >= set(new)
    assert set(new) == {s for s in _ffi.SYMBOLS if s.startswith("w2a_q_")}
    for s in new:
        proto = re.search(r"\b" + s + r"\s*\(([^;]*)\);", header).group(1)
        assert len(proto.split(",")) == len(getattr(lib, s).argtypes), s
    assert lib.w2a_abi_version() == _ffi.ABI_VERSION  # the change is additive
    assert re.search(r"#define W2A_MLP_HEADS_STRIDE", header)
