"""value_gradient() and imitation_gradient(day_weight=...) without a GPU: the fp64 restatement the GPU tests compare the
kernels with (tests/value_gradient_restatement.py) is minus the gradient of 1/2 sum w (V - Q)^2 (torch autograd), the
telescoped route the kernels take is Q_s - V_s, each of three plausible mistakes moves the gradient by more than its
bound, day weights restate to the unweighted imitation result, and the binding and the argument checks refuse what they
must before anything could be launched."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from imitation_restatement import imitation_linear_fp64, imitation_mlp_fp64  # noqa: E402
from test_abi import header_symbols  # noqa: E402
from test_policy_gradient_cpu import _mini  # noqa: E402
from value_gradient_restatement import (telescoped, value_linear_fp64, value_mlp_fp64,  # noqa: E402
                                        weighted_imitation_linear_fp64, weighted_imitation_mlp_fp64)

from weather2alert_amd import _ffi, build, policy  # noqa: E402

NEW = ("w2a_value_gradient_linear_workspace_bytes", "w2a_value_gradient_linear", "w2a_value_gradient_mlp_workspace_bytes",
       "w2a_value_gradient_mlp", "w2a_imitation_gradient_linear_weighted", "w2a_imitation_gradient_mlp_weighted")


def forced_run(V, tup, schedule, S):
    """The oracle forced along `schedule` (bool [n, T], attempts by day of the episode) for S days from a reset: the rows
    held before every decision (S + 1 slabs: the last is the row the call leaves behind), the rewards, the valid days,
    the attempts and the alerts issued."""
    E.oracle_reset(V, tup)
    n = len(tup["budget"])
    R = dict(obs=np.zeros((S + 1, n, V.obs.shape[1])), reward=np.zeros((S, n)), labels=np.zeros((S, n), bool),
             valid=np.zeros((S, n), bool), issued=np.zeros((S, n), bool))
    for s in range(S):
        live = ~V._finished
        R["obs"][s] = V.obs
        lab = schedule[np.arange(n), np.minimum(V.t, schedule.shape[1] - 1)] & live
        r, _, actual, _ = E.oracle_step(V, lab.astype(np.int64))
        R["reward"][s], R["labels"][s], R["valid"][s], R["issued"][s] = np.where(live, r, 0.0), lab, live, live & (actual == 1)
    R["obs"][S] = V.obs
    return R


@pytest.fixture(scope="module")
def mini(golden_dir, mini_root):
    """the committed mini data set, 200 envs with budgets 0..8, a schedule that attempts on 30 % of the days (attempts
    over budget), forced through the oracle for whole episodes and for a truncated 40-day chunk"""
    ct, V, tup = _mini(golden_dir, mini_root)
    n = len(tup["budget"])
    sched = np.random.default_rng(1).random((n, ct.T)) < 0.3
    w = np.random.default_rng(2).standard_normal(n)
    w[::7] = 0.0
    return ct, forced_run(V, tup, sched, ct.T), forced_run(V, tup, sched, 40), w, E.groups(n)


def _torch_loss(R, w, layers, activation, g, G):
    """sum over groups of (1 / N_g) sum_e w_e 1/2 sum_s (V_s - Q_s)^2 in torch fp64; layers as test_imitation_cpu's"""
    valid = torch.as_tensor(R["valid"])
    S = R["valid"].shape[0]
    r = np.where(R["valid"], R["reward"], 0.0)
    Q = torch.as_tensor(np.cumsum(r[::-1], axis=0)[::-1].copy())
    gt = torch.as_tensor(g)
    h = torch.as_tensor(R["obs"][:S])
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
    per_env = 0.5 * torch.where(valid, (z - Q) ** 2, torch.zeros_like(z)).sum(0) * torch.as_tensor(w)
    cnt = torch.as_tensor(np.bincount(g, minlength=G).astype(np.float64))
    return (per_env / cnt[gt]).sum()


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_linear_restatement_descends_the_squared_error(mini):
    ct, whole, chunk, w, g = mini
    W, b = E.linear_params(ct)
    for R in (whole, chunk):
        assert (R["labels"] & ~R["issued"] & R["valid"]).any()  # attempts over budget
        ref = value_linear_fp64(R["obs"], R["valid"], R["reward"], w, W, b, g, E.G)
        Wt = torch.tensor(W.astype(np.float64), requires_grad=True)
        bt = torch.tensor(b.astype(np.float64), requires_grad=True)
        total = _torch_loss(R, w, [(Wt, bt)], None, g, E.G)
        total.backward()
        assert _rel(ref["weight"], -Wt.grad.numpy()) <= 1e-10 and _rel(ref["bias"], -bt.grad.numpy()) <= 1e-10
        assert abs(np.nansum(ref["group_loss"]) - float(total.detach())) <= 1e-10 * abs(float(total.detach()))
        np.testing.assert_array_equal(ref["days"], R["valid"].sum(axis=0))
        np.testing.assert_allclose(ref["ret"], np.where(R["valid"], R["reward"], 0.0).sum(axis=0), rtol=1e-13, atol=1e-13)
        assert (ref["bound"][~np.isnan(ref["bound"])] >= 0).all()


NETS = {"tanh1_o2": ((9,), "tanh", 2), "tanh2_o2": ((7, 13), "tanh", 2), "relu1": ((9,), "relu", 1),
        "relu2_o2": ((7, 13), "relu", 2), "tanh2": ((7, 13), "tanh", 1)}


@pytest.mark.parametrize("name", list(NETS))
def test_mlp_restatement_descends_the_squared_error(mini, name):
    ct, whole, chunk, w, g = mini
    hidden, act, n_out = NETS[name]
    layers = E.net(ct, hidden, n_out, seed=5)
    R = chunk
    ref = value_mlp_fp64(R["obs"], R["valid"], R["reward"], w, layers, act, g, E.G)
    lt = [(torch.tensor(W.astype(np.float64), requires_grad=True), torch.tensor(b.astype(np.float64), requires_grad=True))
          for W, b in layers]
    total = _torch_loss(R, w, lt, act, g, E.G)
    total.backward()
    for (dW, db), (Wt, bt) in zip(ref["layers"], lt):
        assert _rel(dW, -Wt.grad.numpy()) <= 1e-10 and _rel(db, -bt.grad.numpy()) <= 1e-10, name
    assert abs(np.nansum(ref["group_loss"]) - float(total.detach())) <= 1e-10 * abs(float(total.detach()))
    assert all((bW >= 0).all() and (bb >= 0).all() for bW, bb in ref["bound"])


def test_telescoped_sum_is_the_residual(mini):
    """total - prefix of y_s = r_s + V_{s+1} - V_s (V := 0 past the env's last stepped day) is Q_s - V_s, for whole
    episodes of ragged lengths and for a truncated chunk"""
    ct, whole, chunk, w, g = mini
    W, b = E.linear_params(ct)
    for R in (whole, chunk):
        ref = value_linear_fp64(R["obs"], R["valid"], R["reward"], w, W, b, g, E.G)
        A, y = telescoped(R["reward"], ref["V"], R["valid"])
        scale = np.abs(ref["advantage"]).max()
        assert scale > 0 and np.abs(A - ref["advantage"]).max() <= 1e-12 * scale
        np.testing.assert_allclose(y.sum(axis=0), ref["ret"] - ref["V"][0], rtol=0, atol=1e-12 * scale)
    assert chunk["valid"][-1].any()  # the chunk ends before these envs' episodes do: truncated, V := 0 past its last day


def _moved(ref, mut):
    return bool((np.abs(np.concatenate([mut["weight"], mut["bias"][:, None]], axis=1)
                        - np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1)) > ref["bound"]).any())


def _moved_mlp(ref, mut):
    return any((np.abs(m - r) > bd).any() for (mW, mb), (rW, rb), (bW, bb) in zip(mut["layers"], ref["layers"], ref["bound"])
               for m, r, bd in ((mW, rW, bW), (mb, rb, bb)))


def test_mutants_move_the_gradient_beyond_the_bound(mini, golden_dir, mini_root):
    """V_{s+1} dropped from the one-step residual, the value of the row a truncated chunk leaves behind used past its
    last day (bootstrapping), and the attempted instead of the issued alert shown in the next row at the budget: each
    moves some component by more than the bound the GPU tests hold the kernels to. The third is the weakest of the
    three: it flips the alert_lag1 column alone, where a kernel that issued the attempt would also move the remaining
    budget, the 14-day count, the streak and the reward -- the smallest footprint such a fault can have, and the bound
    still sees it. The whole effect is held by tests/test_value_gradient_gpu.py's "attempts" cases against a twin
    stepped through step()."""
    ct, whole, chunk, w, g = mini
    W, b = E.linear_params(ct)
    layers = E.net(ct, (7, 13), 1, seed=5)
    lag = ct.feature_names.index("alert_lag1")
    for moved, fn, par in ((_moved, value_linear_fp64, (W, b)), (_moved_mlp, value_mlp_fp64, (layers, "tanh"))):
        R = chunk
        S = R["valid"].shape[0]
        ref = fn(R["obs"], R["valid"], R["reward"], w, *par, g, E.G)
        A_drop = telescoped(R["reward"], ref["V"], R["valid"], drop_next=True)[0]
        assert moved(ref, fn(R["obs"], R["valid"], R["reward"], w, *par, g, E.G, residual=A_drop))
        # the value of slab S: one more decision's worth of rows, evaluated by the same restatement
        one = np.ones((1, len(w)), bool)
        v_end = fn(R["obs"][S:], one, np.zeros((1, len(w))), None, *par, g, E.G)["V"][0]
        A_boot = telescoped(R["reward"], ref["V"], R["valid"], bootstrap=v_end)[0]
        assert moved(ref, fn(R["obs"], R["valid"], R["reward"], w, *par, g, E.G, residual=A_boot))
        over = R["labels"] & ~R["issued"] & R["valid"]
        assert over[:-1].any()
        obs_att = R["obs"].copy()
        obs_att[1:S + 1, :, lag] = np.where(over, 1.0, obs_att[1:S + 1, :, lag])
        assert moved(ref, fn(obs_att, R["valid"], R["reward"], w, *par, g, E.G))


def test_day_weights_restate_to_the_unweighted_imitation_result(mini):
    """day_weight=None is tests/imitation_restatement.py's result; day_weight of ones equals env_weight of ones; a
    day weight constant per env equals that env_weight"""
    ct, whole, chunk, w, g = mini
    R = chunk
    forced = np.zeros_like(R["valid"])
    W, b = E.linear_params(ct)
    layers = E.net(ct, (7, 13), 2, seed=5)
    ones = np.ones(R["valid"].shape)
    base = imitation_linear_fp64(R["obs"], R["labels"], R["valid"], forced, w, W, b, g, E.G)
    for dw, ww, want in ((None, w, base), (w[None, :] * ones, None, base),
                         (ones, None, imitation_linear_fp64(R["obs"], R["labels"], R["valid"], forced, np.ones(len(w)), W, b, g, E.G))):
        got = weighted_imitation_linear_fp64(R["obs"], R["labels"], R["valid"], forced, ww, dw, W, b, g, E.G)
        np.testing.assert_allclose(got["weight"], want["weight"], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(got["bias"], want["bias"], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(got["bound"], want["bound"], rtol=1e-12, atol=1e-300)
    basem = imitation_mlp_fp64(R["obs"], R["labels"], R["valid"], forced, w, layers, "tanh", g, E.G)
    onem = imitation_mlp_fp64(R["obs"], R["labels"], R["valid"], forced, np.ones(len(w)), layers, "tanh", g, E.G)
    for dw, ww, want in ((None, w, basem), (w[None, :] * ones, None, basem), (ones, None, onem)):
        got = weighted_imitation_mlp_fp64(R["obs"], R["labels"], R["valid"], forced, ww, dw, layers, "tanh", g, E.G)
        for (dW, db), (rW, rb), (bW, bb), (cW, cb) in zip(got["layers"], want["layers"], got["bound"], want["bound"]):
            np.testing.assert_allclose(dW, rW, rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(db, rb, rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(bW, cW, rtol=1e-9, atol=1e-300)
            np.testing.assert_allclose(bb, cb, rtol=1e-9, atol=1e-300)
    # a day weight that differs by day is not an env weight
    dw = np.random.default_rng(3).standard_normal(R["valid"].shape)
    got = weighted_imitation_linear_fp64(R["obs"], R["labels"], R["valid"], forced, w, dw, W, b, g, E.G)
    assert _moved(base, got)


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
    assert lib.w2a_abi_version() == 18 and _ffi.ABI_VERSION == 18


def test_header_and_ffi_signatures_agree():
    """the argument count and the pointer / integer kind of every argument of the new entry points, header against
    _ffi's argtypes"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "w2a.h")).read()
    lib = _ffi.load()
    for name in NEW:
        i = re.search(rf"^(?:size_t|int) {name}\(", text, re.M).end() - len(name) - 2
        args = [a.strip() for a in text[text.index("(", i) + 1:text.index(");", i)].replace("\n", " ").split(",")]
        kinds = []
        for a in args:
            if "*" in a:
                kinds.append("p")
            else:
                kinds.append({"int32_t": "i32", "int64_t": "i64", "size_t": "sz"}[a.split()[0]])
        have = []
        for t in getattr(lib, name).argtypes:
            have.append("p" if (t is C.c_void_p or hasattr(t, "_type_") and not isinstance(t._type_, str)) else
                        {C.c_int32: "i32", C.c_int64: "i64", C.c_size_t: "sz"}[t])
        assert kinds == have, (name, kinds, have)
        ret = text[:i].rsplit("\n", 1)[-1].strip()
        assert (getattr(lib, name).restype is C.c_size_t) == (ret == "size_t") and ret in ("size_t", "int"), name


def _err(lib):
    return lib.w2a_last_error().decode()


def test_bad_arguments_are_refused_on_the_host(lib):
    """NULL and bad arguments return -1 (W2A_ERR_ARG) with a message naming the entry point; nothing is launched (there
    is no device here, and the handle is NULL throughout). The fake pointers are never dereferenced: the handle is
    checked before anything reads them."""
    P = 4096  # a non-NULL, 256-B aligned address that is never read
    lp = _ffi.LinearPolicy()
    lin = lib.w2a_value_gradient_linear
    ok = (P, 5, None, 3, P, P, P, P, P, None, P, 1 << 20, None)  # alert_mask .. stream

    def call(fn, pol, **kw):
        names = ("alert_mask", "mask_words", "env_weight", "n_steps", "obs", "grad", "sq_error", "days", "ret",
                 "advantage", "workspace", "workspace_bytes", "stream")
        a = dict(zip(names, ok))
        a.update(kw)
        return fn(None, pol, *(a[k] for k in names))

    assert call(lin, None) == -1 and "NULL value" in _err(lib)
    lp.weight, lp.bias, lp.n_groups = P, P, 1
    lp.sample, lp.require_budget = 7, 7  # ignored
    assert call(lin, C.byref(lp), n_steps=0) == -1 and "n_steps" in _err(lib)
    assert call(lin, C.byref(lp), alert_mask=None) == -1 and "alert_mask" in _err(lib)
    assert call(lin, C.byref(lp), obs=None) == -1 and "NULL obs" in _err(lib)
    for k in ("grad", "sq_error", "days", "ret"):
        assert call(lin, C.byref(lp), **{k: None}) == -1 and "NULL grad, sq_error, days or ret" in _err(lib)
    assert call(lin, C.byref(lp), workspace=None) == -1 and "NULL workspace" in _err(lib)
    assert call(lin, C.byref(lp), workspace=P + 64) == -1 and "256-B aligned" in _err(lib)
    assert call(lin, C.byref(lp)) == -1 and "NULL handle" in _err(lib)
    lp.weight = P + 4
    assert call(lin, C.byref(lp)) == -1 and "16-B aligned" in _err(lib)
    assert _err(lib).startswith("w2a_value_gradient_linear")

    mp = _ffi.MlpPolicy()
    mlp = lib.w2a_value_gradient_mlp
    assert call(mlp, None) == -1 and "NULL value" in _err(lib)
    mp.params, mp.n_groups, mp.n_layers, mp.width = P, 1, 2, 48
    assert call(mlp, C.byref(mp)) == -1 and "width" in _err(lib)
    mp.width = 64
    assert call(mlp, C.byref(mp), n_steps=0) == -1 and "n_steps" in _err(lib)
    assert call(mlp, C.byref(mp), alert_mask=None) == -1 and "alert_mask" in _err(lib)
    assert call(mlp, C.byref(mp), ret=None) == -1 and "ret" in _err(lib)
    assert call(mlp, C.byref(mp), workspace=None) == -1 and "NULL workspace" in _err(lib)
    assert call(mlp, C.byref(mp), workspace=P + 64) == -1 and "256-B aligned" in _err(lib)
    assert call(mlp, C.byref(mp)) == -1 and "NULL handle" in _err(lib)
    assert _err(lib).startswith("w2a_value_gradient_mlp")
    size = lib.w2a_value_gradient_mlp_workspace_bytes
    assert size(0, 10, 1, 16, 1) == 0 and size(100, 10, 1, 48, 1) == 0 and size(100, 10, 1, 16, 3) == 0
    for shape in ((100, 10, 1, 16, 1), (70_000, 153, 5, 64, 2)):
        assert size(*shape) == lib.w2a_policy_gradient_mlp_workspace_bytes(*shape) > 0 and size(*shape) % 256 == 0
    lsize = lib.w2a_value_gradient_linear_workspace_bytes
    assert lsize(0, 10) == 0 and lsize(100, 0) == 0 and lsize(1000, 153) >= 9 * 1000 * 153 and lsize(1000, 153) % 256 == 0

    # the weighted imitation entry points: the unweighted ones' refusals under their own name, and the day count
    lp.weight = P
    lp.sample = lp.require_budget = 0
    linw = lib.w2a_imitation_gradient_linear_weighted
    assert linw(None, None, P, 5, None, P, 3, 3, P, P, P, P, None) == -1 and "NULL policy" in _err(lib)
    assert linw(None, C.byref(lp), None, 5, None, P, 3, 3, P, P, P, P, None) == -1 and "alert_mask" in _err(lib)
    assert linw(None, C.byref(lp), P, 5, None, P, 2, 3, P, P, P, P, None) == -1 and "day_weight" in _err(lib)
    assert linw(None, C.byref(lp), P, 5, None, None, 0, 3, P, P, P, P, None) == -1 and "NULL handle" in _err(lib)
    assert linw(None, C.byref(lp), P, 5, None, P, 3, 3, P, P, P, P, None) == -1 and "NULL handle" in _err(lib)
    assert _err(lib).startswith("w2a_imitation_gradient_linear_weighted")
    mp.sample = mp.require_budget = 0
    mlpw = lib.w2a_imitation_gradient_mlp_weighted
    assert mlpw(None, C.byref(mp), P, 5, None, P, 2, 3, P, P, P, P, P, 1 << 20, None) == -1 and "day_weight" in _err(lib)
    assert mlpw(None, C.byref(mp), P, 5, None, P, 3, 3, P, P, P, P, P, 1 << 20, None) == -1 and "NULL handle" in _err(lib)
    assert _err(lib).startswith("w2a_imitation_gradient_mlp_weighted")
    # the unweighted entry points keep their names in their messages
    assert lib.w2a_imitation_gradient_linear(None, C.byref(lp), P, 5, None, 3, P, P, P, P, None) == -1
    assert _err(lib).startswith("w2a_imitation_gradient_linear:")


def test_python_argument_checks():
    """policy.check_value_args / check_day_weight: everything value_gradient() and day_weight refuse that is not the
    network itself"""
    n, T, cpu = 6, 40, torch.device("cpu")
    ad = np.zeros((n, T), bool)
    ad[1, 3] = ad[2, 31] = ad[2, 32] = True
    mask, w, steps = policy.check_value_args("mlp", ad, None, None, n, T, cpu)
    assert mask.dtype == torch.int32 and mask.shape == (n, 2) and w is None and steps == T
    assert torch.equal(mask, policy.check_imitation_args("mlp", ad, None, None, n, T, cpu)[0])
    bad = [dict(kind="bernoulli"), dict(kind="never"), dict(kind=None), dict(n_steps=0), dict(n_steps=2.5),
           dict(alert_days=ad[:, :-1]), dict(alert_days=ad[:-1]), dict(alert_days=ad.astype(np.uint8)), dict(alert_days=None),
           dict(env_weight=np.ones(n + 1)), dict(env_weight=np.array([1, 2, np.nan, 4, 5, 6.0])),
           dict(reward_mode="posterior_mean"), dict(fixes={"lag"}), dict(fixes={"budget", "obs"})]
    for kw in bad:
        a = dict(kind="linear", alert_days=ad, env_weight=None, n_steps=None, reward_mode="sampled", fixes=())
        a.update(kw)
        with pytest.raises(ValueError, match="value_gradient"):
            policy.check_value_args(a["kind"], a["alert_days"], a["env_weight"], a["n_steps"], n, T, cpu, a["reward_mode"], a["fixes"])
    policy.check_value_args("linear", ad, np.ones(n), 7, n, T, cpu, "sampled", {"budget"})
    assert policy.check_day_weight(None, 5, n, cpu) is None
    d = policy.check_day_weight(np.ones((7, n)), 5, n, cpu)
    assert d.dtype == torch.float32 and d.shape == (7, n) and d.is_contiguous()
    nan = np.ones((5, n))
    nan[4, 2] = np.nan
    for dw in (np.ones((4, n)), np.ones((5, n + 1)), np.ones(n), np.ones((5, n), np.int64), nan, nan * np.inf, np.full((5, n), 1e39)):
        with pytest.raises(ValueError, match="day_weight"):
            policy.check_day_weight(dw, 5, n, cpu)
