"""imitation_gradient() without a GPU: the fp64 restatement the GPU tests compare the kernels with
(tests/imitation_restatement.py) is the gradient of the weighted log-likelihood (torch autograd, finite differences),
each of four plausible mistakes moves it by more than its bound, the ReLU nets of the GPU cases are rarely near a kink,
and the binding and the argument checks refuse what they must before anything could be launched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from imitation_restatement import attempts_from_schedule, imitation_linear_fp64, imitation_mlp_fp64, log_pi  # noqa: E402
from policy_gradient_mlp_cases import MATRIX, net as case_net  # noqa: E402
from policy_gradient_restatement import forced_days  # noqa: E402
from test_abi import header_symbols  # noqa: E402

from weather2alert_amd import _ffi, build, policy  # noqa: E402

NEW = ("w2a_imitation_gradient_linear", "w2a_imitation_gradient_mlp_workspace_bytes", "w2a_imitation_gradient_mlp")


@pytest.fixture(scope="module")
def tabs():
    return E.make_tables()


def forced_run(V, tup, schedule, S, require_budget):
    """The oracle forced along `schedule` (bool [n, T], attempts by day of the episode) for S days from a reset: the rows
    held before every decision, the attempted actions, the valid / forced days and the alerts issued."""
    E.oracle_reset(V, tup)
    n = len(tup["budget"])
    R = dict(obs=np.zeros((S, n, V.obs.shape[1])), labels=np.zeros((S, n), bool), valid=np.zeros((S, n), bool),
             issued=np.zeros((S, n), bool))
    for s in range(S):
        live = ~V._finished
        R["obs"][s] = V.obs
        lab = schedule[np.arange(n), np.minimum(V.t, schedule.shape[1] - 1)] & live
        act = lab & ~((V.budget - V.used <= 0) if require_budget else False)
        _, _, actual, _ = E.oracle_step(V, act.astype(np.int64))
        R["labels"][s], R["valid"][s], R["issued"][s] = lab, live, live & (actual == 1)
    R["forced"] = forced_days(require_budget, tup["budget"], np.zeros(n, np.int64), R["issued"], R["valid"])
    return R


@pytest.fixture(scope="module")
def run27(tabs):
    """slot27 table (60-day episodes, budget 12), 150 envs, a schedule that attempts on 40 % of the days: attempts over
    budget and, with require_budget, forced days"""
    tb = tabs["slot27"]
    n = 150
    tup = E.host_tuples(tb, n)
    sched = np.random.default_rng(1).random((n, tb.ct.T)) < 0.4
    w = np.random.default_rng(2).standard_normal(n)
    w[::7] = 0.0
    return tb.ct, {rb: forced_run(tb.oracle(), tup, sched, tb.ct.T, rb) for rb in (False, True)}, w, E.groups(n)


def _torch_ll(R, w, layers, activation, g, G, n_out_fold=True):
    """sum over groups of (1 / N_g) sum_e w_e sum_s m_s log pi in torch fp64; layers: list of (W, b) requires-grad tensors
    with a leading G; activation None = linear (layers = [(W [G, n_obs], b [G])])"""
    m = torch.as_tensor(R["valid"] & ~R["forced"])
    gt = torch.as_tensor(g)
    h = torch.as_tensor(R["obs"])
    if activation is None:
        W, b = layers[0]
        z = (h * W[gt][None]).sum(-1) + b[gt][None]
    else:
        f = torch.tanh if activation == "tanh" else torch.relu
        for W, b in layers[:-1]:
            h = f(torch.einsum("snj,nuj->snu", h, W[gt]) + b[gt][None])
        Wo, bo = layers[-1]
        if Wo.shape[1] == 2:  # folded and rounded to f32 once, as the host does; the rounding passes the gradient on
            Wf, bf = Wo[:, 1] - Wo[:, 0], bo[:, 1] - bo[:, 0]
            Wf = Wf + (Wf.detach().float().double() - Wf.detach())
            bf = bf + (bf.detach().float().double() - bf.detach())
        else:
            Wf, bf = Wo[:, 0], bo[:, 0]
        z = (h * Wf[gt][None]).sum(-1) + bf[gt][None]
    lp = policy.action_log_prob(z, torch.as_tensor(R["labels"]))
    per_env = (torch.where(m, lp, torch.zeros_like(lp))).sum(0) * torch.as_tensor(w)
    cnt = torch.as_tensor(np.bincount(g, minlength=G).astype(np.float64))
    return (per_env / cnt[gt]).sum()


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_linear_restatement_is_the_gradient_of_the_log_likelihood(run27):
    ct, runs, w, g = run27
    W, b = E.linear_params(ct)
    for rb, R in runs.items():
        assert (R["labels"] & ~R["issued"] & R["valid"]).any()  # attempts over budget
        assert R["forced"][R["valid"]].any() == rb
        ref = imitation_linear_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, W, b, g, E.G)
        Wt = torch.tensor(W.astype(np.float64), requires_grad=True)
        bt = torch.tensor(b.astype(np.float64), requires_grad=True)
        total = _torch_ll(R, w, [(Wt, bt)], None, g, E.G)
        total.backward()
        assert _rel(ref["weight"], Wt.grad.numpy()) <= 1e-10 and _rel(ref["bias"], bt.grad.numpy()) <= 1e-10
        assert abs(np.nansum(ref["group_ll"]) - float(total.detach())) <= 1e-10 * abs(float(total.detach()))
        m = R["valid"] & ~R["forced"]
        np.testing.assert_array_equal(ref["days"], m.sum(axis=0))
        assert (ref["ll"] <= 0).all() and (ref["ll"][ref["days"] > 0] < 0).all()


NETS = {"tanh1": ((9,), "tanh", 1), "tanh1_o2": ((9,), "tanh", 2), "tanh2": ((7, 13), "tanh", 1),
        "tanh2_o2": ((7, 13), "tanh", 2), "relu1": ((9,), "relu", 1), "relu1_o2": ((9,), "relu", 2),
        "relu2": ((7, 13), "relu", 1), "relu2_o2": ((7, 13), "relu", 2)}


@pytest.mark.parametrize("name", list(NETS))
def test_mlp_restatement_is_the_gradient_of_the_log_likelihood(run27, name):
    ct, runs, w, g = run27
    hidden, act, n_out = NETS[name]
    layers = E.net(ct, hidden, n_out, seed=5)
    R = runs[True]
    ref = imitation_mlp_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, layers, act, g, E.G)
    lt = [(torch.tensor(W.astype(np.float64), requires_grad=True), torch.tensor(b.astype(np.float64), requires_grad=True))
          for W, b in layers]
    total = _torch_ll(R, w, lt, act, g, E.G)
    total.backward()
    for (dW, db), (Wt, bt) in zip(ref["layers"], lt):
        assert _rel(dW, Wt.grad.numpy()) <= 1e-10 and _rel(db, bt.grad.numpy()) <= 1e-10, name
    assert abs(np.nansum(ref["group_ll"]) - float(total.detach())) <= 1e-10 * abs(float(total.detach()))
    assert all((bW >= 0).all() and (bb >= 0).all() for bW, bb in ref["bound"])


def test_restatement_gradient_matches_finite_differences_of_its_own_ll(run27):
    """central differences of sum_g group_ll along random directions, linear and a tanh net"""
    ct, runs, w, g = run27
    R = runs[True]
    rng = np.random.default_rng(0)
    args = (R["obs"], R["labels"], R["valid"], R["forced"], w)
    W, b = (x.astype(np.float64) for x in E.linear_params(ct))
    ref = imitation_linear_fp64(*args, W, b, g, E.G)
    for _ in range(3):
        dW, db = rng.standard_normal(W.shape), rng.standard_normal(b.shape)
        h = 1e-6
        f = lambda s: np.nansum(imitation_linear_fp64(*args, W + s * dW, b + s * db, g, E.G)["group_ll"])  # noqa: E731
        fd = (f(h) - f(-h)) / (2 * h)
        an = (ref["weight"] * dW).sum() + (ref["bias"] * db).sum()
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1.0)
    layers = [(Wl.astype(np.float64), bl.astype(np.float64)) for Wl, bl in E.net(ct, (7, 13), 1, seed=5)]
    refm = imitation_mlp_fp64(*args, layers, "tanh", g, E.G)
    for _ in range(2):
        d = [(rng.standard_normal(Wl.shape), rng.standard_normal(bl.shape)) for Wl, bl in layers]
        d[-1] = (d[-1][0] * 0.0, d[-1][1] * 0.0)  # the output row is rounded to f32 by the fold: no smooth direction
        h = 1e-6
        f = lambda s: np.nansum(imitation_mlp_fp64(*args, [(Wl + s * a, bl + s * c) for (Wl, bl), (a, c) in zip(layers, d)],  # noqa: E731
                                                   "tanh", g, E.G)["group_ll"])
        fd = (f(h) - f(-h)) / (2 * h)
        an = sum((gW * a).sum() + (gb * c).sum() for (gW, gb), (a, c) in zip(refm["layers"], d))
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1.0)


def _moved(ref, mut):
    return bool((np.abs(np.concatenate([mut["weight"], mut["bias"][:, None]], axis=1)
                        - np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1)) > ref["bound"]).any())


def _moved_mlp(ref, mut):
    return any((np.abs(m - r) > bd).any() for (mW, mb), (rW, rb), (bW, bb) in zip(mut["layers"], ref["layers"], ref["bound"])
               for m, r, bd in ((mW, rW, bW), (mb, rb, bb)))


def test_mutants_move_the_gradient_beyond_the_bound(run27):
    """labels shifted by one day, m_s ignored, env_weight dropped, the attempted action replaced by the issued one on
    over-budget days: each moves some component by more than the bound the GPU tests hold the kernels to."""
    ct, runs, w, g = run27
    W, b = E.linear_params(ct)
    layers = E.net(ct, (7, 13), 1, seed=5)
    for moved, fn, par in ((_moved, imitation_linear_fp64, (W, b)), (_moved_mlp, imitation_mlp_fp64, (layers, "tanh"))):
        Rt, Rf = runs[True], runs[False]
        ref = fn(Rt["obs"], Rt["labels"], Rt["valid"], Rt["forced"], w, *par, g, E.G)
        shifted = np.concatenate([Rt["labels"][1:], np.zeros_like(Rt["labels"][:1])]) & Rt["valid"]
        assert moved(ref, fn(Rt["obs"], shifted, Rt["valid"], Rt["forced"], w, *par, g, E.G))
        assert moved(ref, fn(Rt["obs"], Rt["labels"], Rt["valid"], Rt["forced"], w, *par, g, E.G, use_m=False))
        assert moved(ref, fn(Rt["obs"], Rt["labels"], Rt["valid"], Rt["forced"], w, *par, g, E.G, use_w=False))
        reff = fn(Rf["obs"], Rf["labels"], Rf["valid"], Rf["forced"], w, *par, g, E.G)
        assert (Rf["labels"] != Rf["issued"]).any()
        assert moved(reff, fn(Rf["obs"], Rf["issued"], Rf["valid"], Rf["forced"], w, *par, g, E.G))


def test_attempts_from_schedule_follows_each_envs_day():
    sched = np.zeros((3, 10), bool)
    sched[0, 2], sched[1, 5], sched[2, 9] = True, True, True
    valid = np.ones((4, 3), bool)
    valid[2:, 1] = False
    lab = attempts_from_schedule(sched, np.array([0, 4, 6]), valid)
    assert lab[:, 0].tolist() == [False, False, True, False]
    assert lab[:, 1].tolist() == [False, True, False, False]
    assert lab[:, 2].tolist() == [False, False, False, True]
    assert abs(log_pi(0.0, 1) + np.log(2)) < 1e-15 and abs(log_pi(800.0, 0) + 800.0) < 1e-9 and log_pi(800.0, 1) == 0.0


def test_relu_cases_are_rarely_near_a_kink(tabs):
    """The ReLU nets the GPU test runs (tests/policy_gradient_mlp_cases.py), forced along a random schedule on the CPU
    reference alone: under 1 % of the unit-days fall under the near-kink rule that widens the bound."""
    tb = tabs["slot27"]
    n = 200
    tup = E.host_tuples(tb, n)
    sched = np.random.default_rng(3).random((n, tb.ct.T)) < 0.3
    R = forced_run(tb.oracle(), tup, sched, tb.ct.T, False)
    g = E.groups(n)
    for name, (_, hidden, act, n_out) in MATRIX.items():
        if act != "relu":
            continue
        ref = imitation_mlp_fp64(R["obs"], R["labels"], R["valid"], R["forced"], None,
                                 case_net(tb.ct, name, hidden, n_out), act, g, E.G)
        print(f"{name}: near-kink fraction {ref['near_kink']:.2e}")
        assert ref["near_kink"] < 0.01, name


# ---------------------------------------------------------------------------------------------------- binding
@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


def test_header_and_symbols_agree(lib):
    syms = header_symbols()
    assert syms == sorted(_ffi.SYMBOLS)
    for s in NEW:
        assert s in syms and hasattr(lib, s), s
    assert lib.w2a_abi_version() == 18


def _err(lib):
    return lib.w2a_last_error().decode()


def test_bad_arguments_are_refused_on_the_host(lib):
    """NULL and bad arguments return -1 (W2A_ERR_ARG) with a message naming the entry point; nothing is launched (there
    is no device here, and the handle is NULL throughout). The fake pointers are never dereferenced: the handle is
    checked before anything reads them."""
    P = 4096  # a non-NULL, 256-B aligned address that is never read
    lp = _ffi.LinearPolicy()
    lin = lib.w2a_imitation_gradient_linear
    assert lin(None, None, P, 5, None, 3, P, P, P, P, None) == -1 and "NULL policy" in _err(lib)
    lp.weight, lp.bias, lp.n_groups = P, P, 1
    assert lin(None, C.byref(lp), P, 5, None, 0, P, P, P, P, None) == -1 and "n_steps" in _err(lib)
    assert lin(None, C.byref(lp), None, 5, None, 3, P, P, P, P, None) == -1 and "alert_mask" in _err(lib)
    assert lin(None, C.byref(lp), P, 5, None, 3, None, P, P, P, None) == -1 and "NULL obs" in _err(lib)
    for outs in ((None, P, P), (P, None, P), (P, P, None)):
        assert lin(None, C.byref(lp), P, 5, None, 3, P, *outs, None) == -1 and "NULL grad, loglik or days" in _err(lib)
    assert lin(None, C.byref(lp), P, 5, None, 3, P, P, P, P, None) == -1 and "NULL handle" in _err(lib)
    lp.weight = P + 4
    assert lin(None, C.byref(lp), P, 5, None, 3, P, P, P, P, None) == -1 and "16-B aligned" in _err(lib)
    lp.weight, lp.require_budget = P, 2
    assert lin(None, C.byref(lp), P, 5, None, 3, P, P, P, P, None) == -1 and "require_budget" in _err(lib)
    assert _err(lib).startswith("w2a_imitation_gradient_linear")

    mp = _ffi.MlpPolicy()
    mlp = lib.w2a_imitation_gradient_mlp
    assert mlp(None, None, P, 5, None, 3, P, P, P, P, P, 1 << 20, None) == -1 and "NULL policy" in _err(lib)
    mp.params, mp.n_groups, mp.n_layers, mp.width = P, 1, 2, 48
    assert mlp(None, C.byref(mp), P, 5, None, 3, P, P, P, P, P, 1 << 20, None) == -1 and "width" in _err(lib)
    mp.width = 64
    assert mlp(None, C.byref(mp), P, 5, None, 0, P, P, P, P, P, 1 << 20, None) == -1 and "n_steps" in _err(lib)
    assert mlp(None, C.byref(mp), None, 5, None, 3, P, P, P, P, P, 1 << 20, None) == -1 and "alert_mask" in _err(lib)
    assert mlp(None, C.byref(mp), P, 5, None, 3, P, P, None, P, P, 1 << 20, None) == -1 and "loglik" in _err(lib)
    assert mlp(None, C.byref(mp), P, 5, None, 3, P, P, P, P, None, 1 << 20, None) == -1 and "NULL workspace" in _err(lib)
    assert mlp(None, C.byref(mp), P, 5, None, 3, P, P, P, P, P + 64, 1 << 20, None) == -1 and "256-B aligned" in _err(lib)
    assert mlp(None, C.byref(mp), P, 5, None, 3, P, P, P, P, P, 1 << 20, None) == -1 and "NULL handle" in _err(lib)
    assert _err(lib).startswith("w2a_imitation_gradient_mlp")
    size = lib.w2a_imitation_gradient_mlp_workspace_bytes
    assert size(0, 10, 1, 16, 1) == 0 and size(100, 10, 1, 48, 1) == 0 and size(100, 10, 1, 16, 3) == 0
    for shape in ((100, 10, 1, 16, 1), (70_000, 153, 5, 64, 2)):
        assert size(*shape) == lib.w2a_policy_gradient_mlp_workspace_bytes(*shape) > 0 and size(*shape) % 256 == 0


def test_python_argument_checks():
    """policy.check_imitation_args: everything imitation_gradient() refuses that is not the policy itself"""
    n, T, cpu = 6, 40, torch.device("cpu")
    ad = np.zeros((n, T), bool)
    ad[1, 3] = ad[2, 31] = ad[2, 32] = ad[5, 39] = True
    mask, w, steps = policy.check_imitation_args("linear", ad, None, None, n, T, cpu)
    assert mask.dtype == torch.int32 and mask.shape == (n, 2) and w is None and steps == T
    words = mask.numpy().view(np.uint32)
    assert words[1, 0] == 1 << 3 and words[2, 0] == 1 << 31 and words[2, 1] == 1 and words[5, 1] == 1 << 7
    assert words.sum() == (1 << 3) + (1 << 31) + 1 + (1 << 7)
    mask2, w2, steps2 = policy.check_imitation_args("mlp", torch.as_tensor(ad), np.arange(n, dtype=np.float64) - 2, 7, n, T, cpu)
    assert torch.equal(mask2, mask) and w2.dtype == torch.float32 and w2.tolist() == [-2, -1, 0, 1, 2, 3] and steps2 == 7
    bad = [dict(kind="bernoulli"), dict(kind=None), dict(n_steps=0), dict(n_steps=-3), dict(n_steps=2.5),
           dict(alert_days=ad.astype(np.uint8)), dict(alert_days=ad[:, :-1]), dict(alert_days=ad[:-1]),
           dict(alert_days=ad[0]), dict(alert_days=None), dict(env_weight=np.ones(n, np.int64)),
           dict(env_weight=np.ones(n + 1)), dict(env_weight=np.ones((n, 1))),
           dict(env_weight=np.array([1, 2, np.nan, 4, 5, 6.0])), dict(env_weight=np.array([1, 2, np.inf, 4, 5, 6.0])),
           dict(env_weight=np.array([1, 2, 1e39, 4, 5, 6.0])), dict(fixes={"lag"}), dict(fixes={"budget", "obs"})]
    for kw in bad:
        a = dict(kind="linear", alert_days=ad, env_weight=None, n_steps=None, fixes=())
        a.update(kw)
        with pytest.raises(ValueError):
            policy.check_imitation_args(a["kind"], a["alert_days"], a["env_weight"], a["n_steps"], n, T, cpu, a["fixes"])
    policy.check_imitation_args("linear", ad, None, None, n, T, cpu, fixes={"budget"})
