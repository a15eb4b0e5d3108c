"""value_gradient(gamma=, gae_lambda=, bootstrap=, value_target=, target=) without a GPU, on the oracle's trajectory of
tests/golden/mini: the fp64 restatement the GPU tests compare the kernels with (tests/gae_restatement.py) is minus the
torch-autograd gradient of 1/2 sum w (V - stopgrad(R))^2 with R from an independently written SB3-style backward loop;
(1, 1, no bootstrap) is the critic's own restatement; lambda = 0 leaves the one-step residual; fixed targets reproduce
the call that made them; four plausible mistakes leave the bound; and the binding and the argument checks refuse what
they must before anything could be launched."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from gae_restatement import gae_linear_fp64, gae_mlp_fp64, sb3_style_gae  # noqa: E402
from test_abi import header_symbols  # noqa: E402
from test_policy_gradient_cpu import _mini  # noqa: E402
from test_value_gradient_cpu import forced_run  # noqa: E402
from value_gradient_restatement import value_linear_fp64, value_mlp_fp64  # noqa: E402

from weather2alert_amd import _ffi, build, policy  # noqa: E402

NEW = ("w2a_value_gradient_linear_gae_workspace_bytes", "w2a_value_gradient_linear_gae",
       "w2a_value_gradient_mlp_gae_workspace_bytes", "w2a_value_gradient_mlp_gae")
GL = [(1.0, 1.0), (0.99, 0.95), (0.9, 0.0), (0.0, 0.5)]
NETS = {"linear": None, "relu1": ((9,), "relu", 1), "tanh2": ((7, 13), "tanh", 1), "tanh1_o2": ((9,), "tanh", 2)}


def _ragged_run(V, tup, schedule, S, n_days):
    """forced_run with the oracle's episode lengths replaced after the reset"""
    E.oracle_reset(V, tup)
    V.n_days = np.asarray(n_days, np.int64).copy()
    n = len(tup["budget"])
    R = dict(obs=np.zeros((S + 1, n, V.obs.shape[1])), reward=np.zeros((S, n)), valid=np.zeros((S, n), bool))
    for s in range(S):
        live = ~V._finished
        R["obs"][s] = V.obs
        lab = schedule[np.arange(n), np.minimum(V.t, schedule.shape[1] - 1)] & live
        r = E.oracle_step(V, lab.astype(np.int64))[0]
        R["reward"][s], R["valid"][s] = np.where(live, r, 0.0), live
    R["obs"][S] = V.obs
    return R, ~np.asarray(V._finished).astype(bool)


@pytest.fixture(scope="module")
def mini(golden_dir, mini_root):
    """the committed mini data set, 200 envs with budgets 0..8 and a schedule that attempts on 30 % of the days, forced
    through the oracle for 1 day, 3 days and whole episodes; with every run, which envs are still running after it"""
    ct, V, tup = _mini(golden_dir, mini_root)
    n = len(tup["budget"])
    sched = np.random.default_rng(1).random((n, ct.T)) < 0.3
    w = np.random.default_rng(2).standard_normal(n)
    w[::7] = 0.0
    runs = {}
    for S in (1, 3, ct.T):
        R = forced_run(V, tup, sched, S)
        runs[S] = (R, ~np.asarray(V._finished).astype(bool))
    # the mini set's episodes all last T days: end every env's episode up to 44 days early for ragged lengths
    runs["ragged"] = _ragged_run(V, tup, sched, ct.T, np.asarray(tup["n_days"]) - 11 * (np.arange(n) % 5))
    whole = runs["ragged"][0]["valid"].sum(axis=0)
    assert len(np.unique(whole)) == 5 and not runs[ct.T][1].any() and runs[3][1].all()  # chunks truncate, episodes end
    return ct, runs, w, E.groups(n)


def _params(ct, name):
    if NETS[name] is None:
        return None
    hidden, act, n_out = NETS[name]
    return E.net(ct, hidden, n_out, seed=5), act


def _restate(name, ct, R, alive, w, g, par, **kw):
    if par is None:
        W, b = E.linear_params(ct)
        return gae_linear_fp64(R["obs"], R["valid"], R["reward"], alive, w, W, b, g, E.G, **kw)
    return gae_mlp_fp64(R["obs"], R["valid"], R["reward"], alive, w, par[0], par[1], g, E.G, **kw)


def _flat(ref):
    if "weight" in ref:
        return [(np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1), ref["bound"])]
    return [(x, bd) for (dW, db), (bW, bb) in zip(ref["layers"], ref["bound"]) for x, bd in ((dW, bW), (db, bb))]


def _torch_values(obs, layers, activation, g):
    """z of every slab in torch fp64; layers as tests/test_value_gradient_cpu.py's _torch_loss takes them"""
    gt = torch.as_tensor(g)
    h = torch.as_tensor(obs)
    if activation is None:
        W, b = layers[0]
        return (h * W[gt][None]).sum(-1) + b[gt][None]
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
    return (h * Wf[gt][None]).sum(-1) + bf[gt][None]


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("name", list(NETS))
def test_restatement_is_autograd_of_the_sb3_style_targets(mini, name):
    """minus the gradient of sum_g (1 / N_g) sum_e w_e 1/2 sum_s (V_s - stopgrad(R_s))^2, R_s = last_gae_lam + V_s from
    the SB3-style loop, at every (gamma, lambda), bootstrap on and off, n_steps 1 / 3 / whole"""
    ct, runs, w, g = mini
    par = _params(ct, name)
    if par is None:
        W, b = E.linear_params(ct)
        raw, act = [(W, b)], None
    else:
        raw, act = par
    cnt = torch.as_tensor(np.bincount(g, minlength=E.G).astype(np.float64))
    for key, (R, alive) in runs.items():
        valid = R["valid"]
        S = valid.shape[0]
        for gamma, lam in GL:
            for boot in (False, True):
                ref = _restate(name, ct, R, alive, w, g, par, gamma=gamma, lam=lam, bootstrap=boot)
                lt = [(torch.tensor(np.asarray(Wl, np.float64), requires_grad=True),
                       torch.tensor(np.asarray(bl, np.float64), requires_grad=True)) for Wl, bl in raw]
                z = _torch_values(R["obs"][:S + 1], lt, act, g)
                zn = z.detach().numpy()
                adv, ret = sb3_style_gae(np.where(valid, R["reward"], 0.0), zn[:S], zn[S], valid, alive, gamma, lam, boot)
                per_env = 0.5 * torch.where(torch.as_tensor(valid), (z[:S] - torch.as_tensor(ret)) ** 2,
                                            torch.zeros_like(z[:S])).sum(0) * torch.as_tensor(w)
                total = (per_env / cnt[torch.as_tensor(g)]).sum()
                total.backward()
                what = (name, S, gamma, lam, boot)
                scale = max(np.abs(adv).max(), 1e-300)
                assert np.abs(ref["advantage"] - adv).max() <= 1e-12 * scale, what
                assert np.abs(ref["value_target"] - ret).max() <= 1e-12 * max(np.abs(ret).max(), scale), what
                if "weight" in ref:  # (weight | bias) side by side
                    want = [np.concatenate([-lt[0][0].grad.numpy(), -lt[0][1].grad.numpy()[:, None]], axis=1)]
                else:
                    want = [-x.grad.numpy() for pair in lt for x in pair]
                for (got, bound), wnt in zip(_flat(ref), want):
                    assert _rel(got, wnt) <= 1e-10, what
                    assert (bound[~np.isnan(bound)] >= 0).all(), what
                assert abs(np.nansum(ref["group_loss"]) - float(total.detach())) <= 1e-10 * abs(float(total.detach())), what
                np.testing.assert_array_equal(ref["days"], valid.sum(axis=0))


@pytest.mark.parametrize("name", ["linear", "tanh2", "tanh1_o2"])
def test_unit_gamma_and_lambda_without_bootstrap_is_the_critic(mini, name):
    """(1, 1, bootstrap=False) equals value_linear_fp64 / value_mlp_fp64 to 1e-12 relative, whole episodes and chunks"""
    ct, runs, w, g = mini
    par = _params(ct, name)
    for S, (R, alive) in runs.items():
        ref = _restate(name, ct, R, alive, w, g, par)
        if par is None:
            W, b = E.linear_params(ct)
            old = value_linear_fp64(R["obs"], R["valid"], R["reward"], w, W, b, g, E.G)
        else:
            old = value_mlp_fp64(R["obs"], R["valid"], R["reward"], w, par[0], par[1], g, E.G)
        for (x, _), (y, _) in zip(_flat(ref), _flat(old)):
            assert _rel(x, y) <= 1e-12, (name, S)
        for k in ("advantage", "sq", "ret"):
            assert _rel(ref[k], old[k]) <= 1e-12, (name, S, k)
        # Q_s = R_s at (1, 1): the lambda-return is the reward-to-go
        Q = np.cumsum(np.where(R["valid"], R["reward"], 0.0)[::-1], axis=0)[::-1]
        assert np.abs(ref["value_target"] - Q * R["valid"]).max() <= 1e-12 * np.abs(Q).max(), (name, S)


def test_lambda_zero_leaves_the_one_step_residual(mini):
    ct, runs, w, g = mini
    for S, (R, alive) in runs.items():
        for boot in (False, True):
            ref = _restate("linear", ct, R, alive, w, g, None, gamma=0.9, lam=0.0, bootstrap=boot)
            np.testing.assert_array_equal(ref["advantage"], ref["delta"])
            nxt = np.concatenate([ref["V"][1:], (ref["V_last"] * alive * boot)[None, :]], axis=0)
            want = np.where(R["valid"], R["reward"] + 0.9 * nxt - ref["V"], 0.0)
            assert np.abs(ref["advantage"] - want).max() <= 1e-12 * np.abs(want).max()
    assert (runs[3][0]["valid"][2] & runs[3][1]).any()  # a truncated chunk: the bootstrap term is there


@pytest.mark.parametrize("name", ["linear", "tanh2"])
def test_fixed_targets_reproduce_the_call_that_made_them(mini, name):
    ct, runs, w, g = mini
    par = _params(ct, name)
    R, alive = runs[ct.T]
    first = _restate(name, ct, R, alive, w, g, par, gamma=0.99, lam=0.95)
    again = _restate(name, ct, R, alive, w, g, par, target=first["value_target"])
    for (x, _), (y, _) in zip(_flat(again), _flat(first)):
        assert _rel(x, y) <= 1e-12
    assert _rel(again["sq"], first["sq"]) <= 1e-12 and "ret" not in again
    moved = _restate(name, ct, R, alive, w, g, par, target=first["value_target"] + 1.0)
    assert any((np.abs(x - y) > bd).any() for (x, _), (y, bd) in zip(_flat(moved), _flat(first)))


def _leaves(ref, mut):
    return any((np.abs(x - y)[~np.isnan(bd)] > bd[~np.isnan(bd)]).any() for (x, _), (y, bd) in zip(_flat(mut), _flat(ref)))


@pytest.mark.parametrize("name", ["linear", "tanh2"])
def test_mutants_leave_the_bound(mini, name):
    """gamma dropped from Vn_s; the recursion decayed by lambda alone; the row after the episode's terminal day read as
    a bootstrap; the recursion started from the call's last day instead of the env's own (ragged lengths): each moves
    some component of the gradient by more than the bound the GPU tests hold the kernels to"""
    ct, runs, w, g = mini
    par = _params(ct, name)
    for mutant, kw in (("gamma_dropped", dict(gamma=0.9, lam=0.8)), ("lambda_only", dict(gamma=0.9, lam=0.8)),
                       ("terminal_bootstrap", dict(gamma=0.99, lam=0.95, bootstrap=True)),
                       ("call_end_start", dict(gamma=0.99, lam=0.95))):
        R, alive = runs["ragged" if mutant == "call_end_start" else ct.T]
        ref = _restate(name, ct, R, alive, w, g, par, **kw)
        assert not _leaves(ref, _restate(name, ct, R, alive, w, g, par, **kw)), mutant
        assert _leaves(ref, _restate(name, ct, R, alive, w, g, par, mutant=mutant, **kw)), mutant


# ---------------------------------------------------------------------------------------------------- binding
@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


def test_header_symbols_and_signatures_agree(lib):
    syms = header_symbols()
    assert syms == sorted(_ffi.SYMBOLS)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "w2a.h")).read()
    for name in NEW:
        assert name in syms and hasattr(lib, name), name
        i = re.search(rf"^(?:size_t|int) {name}\(", text, re.M).end() - len(name) - 2
        args = [a.strip() for a in text[text.index("(", i) + 1:text.index(");", i)].replace("\n", " ").split(",")]
        kinds = ["p" if "*" in a else {"int32_t": "i32", "int64_t": "i64", "size_t": "sz", "double": "f64"}[a.split()[0]]
                 for a in args]
        have = ["p" if (t is C.c_void_p or hasattr(t, "_type_") and not isinstance(t._type_, str)) else
                {C.c_int32: "i32", C.c_int64: "i64", C.c_size_t: "sz", C.c_double: "f64"}[t]
                for t in getattr(lib, name).argtypes]
        assert kinds == have, (name, kinds, have)
    assert lib.w2a_abi_version() == 18 and _ffi.ABI_VERSION == 18  # additions only


def _err(lib):
    return lib.w2a_last_error().decode()


def test_bad_arguments_are_refused_on_the_host(lib):
    """The refusals of w2a_value_gradient_linear / _mlp in their order under the new names, then gamma, lambda,
    bootstrap, the targets' day count and what targets cannot be combined with -- all W2A_ERR_ARG before the handle is
    looked at (it is NULL throughout, and the fake pointers are never dereferenced)."""
    P = 4096  # a non-NULL, 256-B aligned address that is never read
    names = ("alert_mask", "mask_words", "env_weight", "n_steps", "obs", "grad", "sq_error", "days", "ret", "advantage",
             "gamma", "lam", "bootstrap", "value_target", "target", "target_days", "workspace", "workspace_bytes", "stream")
    ok = (P, 5, None, 3, P, P, P, P, P, None, 0.99, 0.95, 1, None, None, 0, P, 1 << 20, None)

    def call(fn, pol, **kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return fn(None, pol, *(a[k] for k in names))

    lp = _ffi.LinearPolicy()
    lp.weight, lp.bias, lp.n_groups = P, P, 1
    mp = _ffi.MlpPolicy()
    mp.params, mp.n_groups, mp.n_layers, mp.width = P, 1, 2, 64
    for fn, pol, who in ((lib.w2a_value_gradient_linear_gae, lp, "w2a_value_gradient_linear_gae"),
                         (lib.w2a_value_gradient_mlp_gae, mp, "w2a_value_gradient_mlp_gae")):
        assert call(fn, None) == -1 and "NULL value" in _err(lib)
        ref = C.byref(pol)
        assert call(fn, ref, n_steps=0) == -1 and "n_steps" in _err(lib)
        assert call(fn, ref, alert_mask=None) == -1 and "alert_mask" in _err(lib)
        assert call(fn, ref, obs=None) == -1 and "NULL obs" in _err(lib)
        for k in ("grad", "sq_error", "days", "ret"):
            assert call(fn, ref, **{k: None}) == -1 and "NULL grad, sq_error, days or ret" in _err(lib)
        for bad in (-0.01, 1.01, float("nan"), float("inf")):
            assert call(fn, ref, gamma=bad) == -1 and "gamma" in _err(lib)
            assert call(fn, ref, lam=bad) == -1 and "lambda" in _err(lib)
        assert call(fn, ref, bootstrap=2) == -1 and "bootstrap" in _err(lib)
        tg = dict(target=P, target_days=3, gamma=1.0, lam=1.0, bootstrap=0)
        assert call(fn, ref, **dict(tg, target_days=2)) == -1 and "fewer call-days" in _err(lib)
        assert call(fn, ref, **dict(tg, advantage=P)) == -1 and "not formed" in _err(lib)
        assert call(fn, ref, **dict(tg, value_target=P)) == -1 and "not formed" in _err(lib)
        for k, v in (("gamma", 0.5), ("lam", 0.5), ("bootstrap", 1)):
            assert call(fn, ref, **dict(tg, **{k: v})) == -1 and "no meaning" in _err(lib)
        # the refusals above come before these, which come before the handle
        assert call(fn, ref, gamma=2.0, workspace=None) == -1 and "gamma" in _err(lib)
        assert call(fn, ref, workspace=None) == -1 and "NULL workspace" in _err(lib)
        assert call(fn, ref, workspace=P + 64) == -1 and "256-B aligned" in _err(lib)
        for kw in ({}, tg, dict(gamma=0.0, lam=0.0), dict(value_target=P, advantage=P)):
            assert call(fn, ref, **kw) == -1 and "NULL handle" in _err(lib)
        assert _err(lib).startswith(who + ":")
    lp.weight = P + 4
    assert call(lib.w2a_value_gradient_linear_gae, C.byref(lp)) == -1 and "16-B aligned" in _err(lib)
    mp.width = 48
    assert call(lib.w2a_value_gradient_mlp_gae, C.byref(mp)) == -1 and "width" in _err(lib)
    size = lib.w2a_value_gradient_mlp_gae_workspace_bytes
    assert size(0, 10, 1, 16, 1) == 0 and size(100, 10, 1, 48, 1) == 0
    for shape in ((100, 10, 1, 16, 1), (70_000, 153, 5, 64, 2)):
        assert size(*shape) == lib.w2a_value_gradient_mlp_workspace_bytes(*shape) > 0
    lsize = lib.w2a_value_gradient_linear_gae_workspace_bytes
    assert lsize(0, 10) == 0 and lsize(100, 0) == 0 and lsize(1000, 153) % 256 == 0
    assert 17 * 1000 * 153 <= lsize(1000, 153) < 17 * 1000 * 153 + 3 * 256  # 17 B per env-day


def test_python_argument_checks():
    """policy.check_gae_args: gamma and gae_lambda finite in [0, 1], bootstrap and value_target plain bools, target as
    surrogate_gradient()'s advantage and combined with nothing it has no meaning with"""
    n, cpu = 6, torch.device("cpu")
    base = dict(gamma=1.0, gae_lambda=1.0, bootstrap=False, value_target=False, advantage=False, target=None)

    def check(**kw):
        a = dict(base, **kw)
        return policy.check_gae_args(a["gamma"], a["gae_lambda"], a["bootstrap"], a["value_target"], a["advantage"],
                                     a["target"], 5, n, cpu)

    assert check() == (1.0, 1.0, None, False) and check(advantage=True)[3] is False  # today's call, today's kernels
    assert check(gamma=1, gae_lambda=np.float32(1.0))[3] is False
    for kw in (dict(gamma=0.99), dict(gae_lambda=0.0), dict(bootstrap=True), dict(value_target=True),
               dict(target=np.zeros((5, n)))):
        assert check(**kw)[3], kw
    g, lam, tg, new = check(target=np.ones((7, n)))
    assert tg.dtype == torch.float32 and tuple(tg.shape) == (7, n) and tg.is_contiguous() and new
    nan = np.ones((5, n))
    nan[4, 2] = np.nan
    bad = [dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(gamma=True),
           dict(gamma="0.9"), dict(gamma=None), dict(gae_lambda=-1e-9), dict(gae_lambda=2), dict(gae_lambda=float("nan")),
           dict(bootstrap=1), dict(bootstrap=None), dict(value_target=1), dict(value_target="yes"),
           dict(target=np.ones((4, n))), dict(target=np.ones((5, n + 1))), dict(target=np.ones(n)),
           dict(target=np.ones((5, n), np.int64)), dict(target=nan),
           dict(target=np.ones((5, n)), advantage=True), dict(target=np.ones((5, n)), value_target=True),
           dict(target=np.ones((5, n)), gamma=0.9), dict(target=np.ones((5, n)), gae_lambda=0.9),
           dict(target=np.ones((5, n)), bootstrap=True)]
    for kw in bad:
        with pytest.raises(ValueError, match="value_gradient"):
            check(**kw)
