"""surrogate_gradient() without a GPU, on the oracle's trajectory of tests/golden/mini: the fp64 restatement the GPU
tests compare the kernels with (tests/surrogate_restatement.py) is the gradient torch autograd gives for
mean_e w_e sum_s [min(rho A, clamp(rho) A) + beta H] with the ratio built by autograd, it reduces to the weighted
imitation restatement without old log-probabilities and entropy bonus, each of four plausible mistakes moves it by more
than its bound, its clip-edge rule stays under the 1 % cap, and the binding and the argument checks refuse what they must
before anything could be launched."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from imitation_restatement import log_pi  # noqa: E402
from surrogate_restatement import AMBIGUOUS_CAP, entropy, surrogate_linear_fp64, surrogate_mlp_fp64  # noqa: E402
from test_abi import header_symbols  # noqa: E402
from test_imitation_cpu import forced_run  # noqa: E402
from test_policy_gradient_cpu import _mini  # noqa: E402
from value_gradient_restatement import weighted_imitation_linear_fp64, weighted_imitation_mlp_fp64  # noqa: E402

from weather2alert_amd import _ffi, build, policy  # noqa: E402

NEW = ("w2a_surrogate_gradient_linear", "w2a_surrogate_gradient_mlp_workspace_bytes", "w2a_surrogate_gradient_mlp")
CLIP, BETA = 0.2, 0.01


@pytest.fixture(scope="module")
def mini(golden_dir, mini_root):
    """the committed mini data set, 200 envs with budgets 0..8, a schedule that attempts on 30 % of the days (attempts
    over budget; forced days under require_budget), forced through the oracle for a truncated 40-day chunk; weights
    with zeros and negative values, an advantage with zeros and both signs"""
    ct, V, tup = _mini(golden_dir, mini_root)
    n = len(tup["budget"])
    sched = np.random.default_rng(1).random((n, ct.T)) < 0.3
    w = np.random.default_rng(2).standard_normal(n)
    w[::7] = 0.0
    S = 40
    A = np.random.default_rng(3).standard_normal((S, n)).astype(np.float32).astype(np.float64)
    A[:, ::11] = 0.0
    return ct, {rb: forced_run(V, tup, sched, S, rb) for rb in (False, True)}, w, A, E.groups(n)


def _perturbed(params, seed, size):
    """a copy of f32 parameter arrays moved by `size` times a standard normal draw of their own scale"""
    rng = np.random.default_rng(seed)
    return [(x + size * np.abs(x).mean() * rng.standard_normal(x.shape)).astype(np.float32) for x in params]


def _old_linear(ct, R, g, seed=7, size=0.25):
    """old log-probabilities [S, N] as f32: those of the schedule under a perturbed copy of the linear policy"""
    W, b = _perturbed(E.linear_params(ct), seed, size)
    z = np.einsum("snj,nj->sn", R["obs"], W.astype(np.float64)[g]) + b.astype(np.float64)[g][None, :]
    return log_pi(z, R["labels"]).astype(np.float32)


def _torch_z(R, layers, activation, gt):
    """the logit [S, N] in torch fp64; layers: list of (W, b) tensors with a leading G; activation None = linear"""
    h = torch.as_tensor(R["obs"])
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


def _torch_objective(R, w, A, old, clip, beta, layers, activation, g, G):
    """sum over groups of (1 / N_g) sum_e w_e sum_s m_s [min(rho A, clamp(rho, 1 - clip, 1 + clip) A) + beta H] in torch
    fp64, the ratio rho = exp(log pi_theta - old) built by autograd; also the per-env surrogate, kl and entropy sums"""
    m = torch.as_tensor(R["valid"] & ~R["forced"])
    gt = torch.as_tensor(g)
    z = _torch_z(R, layers, activation, gt)
    lp = policy.action_log_prob(z, torch.as_tensor(R["labels"]))
    d = lp - torch.as_tensor(old) if old is not None else lp - lp.detach()
    rho = torch.exp(d)
    At = torch.as_tensor(A)
    surr = torch.min(rho * At, rho.clamp(1.0 - clip, 1.0 + clip) * At)
    ls = torch.nn.functional.logsigmoid  # (softplus() goes linear past its threshold of 20: 2e-9 off)
    H = -(torch.sigmoid(z) * ls(z) + torch.sigmoid(-z) * ls(-z))
    zero = torch.zeros_like(z)
    L, kl, Hs = (torch.where(m, x, zero).sum(0) for x in (surr, (rho - 1.0) - d, H))
    cnt = torch.as_tensor(np.bincount(g, minlength=G).astype(np.float64))
    return ((L + beta * Hs) * torch.as_tensor(w) / cnt[gt]).sum(), L.detach().numpy(), kl.detach().numpy(), Hs.detach().numpy()


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _clips_both_ways(ref, A, what):
    """at least one clipped and one live scored day for each sign of A; the ambiguous share under the cap"""
    scored = ref["m"]
    for sign in (1, -1):
        side = scored & (sign * A > 0)
        assert (side & ~ref["live"]).any() and (side & ref["live"]).any(), (what, sign)
    assert ref["ambiguous_share"] <= AMBIGUOUS_CAP, (what, ref["ambiguous_share"])


def test_linear_restatement_is_the_gradient_of_the_clipped_surrogate(mini):
    ct, runs, w, A, g = mini
    W, b = E.linear_params(ct)
    for rb, R in runs.items():
        assert (R["labels"] & ~R["issued"] & R["valid"]).any()  # attempts over budget
        assert R["forced"][R["valid"]].any() == rb
        old = _old_linear(ct, R, g).astype(np.float64)
        for o_, beta in ((old, BETA), (old, 0.0), (None, BETA)):
            ref = surrogate_linear_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, A, o_, CLIP, beta, W, b, g, E.G)
            Wt = torch.tensor(W.astype(np.float64), requires_grad=True)
            bt = torch.tensor(b.astype(np.float64), requires_grad=True)
            total, L, kl, H = _torch_objective(R, w, A, o_, CLIP, beta, [(Wt, bt)], None, g, E.G)
            total.backward()
            assert _rel(ref["weight"], Wt.grad.numpy()) <= 1e-10 and _rel(ref["bias"], bt.grad.numpy()) <= 1e-10
            np.testing.assert_allclose(ref["L"], L, rtol=1e-9, atol=1e-9)  # two fp64 log-sigmoids, their difference times rho
            np.testing.assert_allclose(ref["kl"], kl, rtol=1e-9, atol=1e-13)
            np.testing.assert_allclose(ref["H"], H, rtol=1e-12, atol=1e-12)
            mm = R["valid"] & ~R["forced"]
            np.testing.assert_array_equal(ref["days"], mm.sum(axis=0))
            assert (ref["kl"] >= -1e-12).all() and (ref["H"] >= 0).all() and (ref["bound"][~np.isnan(ref["bound"])] >= 0).all()
            if o_ is not None:
                _clips_both_ways(ref, A, f"linear rb={rb}")
                assert (ref["clipped"] > 0).any()
            else:
                assert (ref["clipped"] == 0).all() and (ref["kl"] == 0).all() and ref["ambiguous_share"] == 0.0


NETS = {"tanh1": ((9,), "tanh", 1), "tanh1_o2": ((9,), "tanh", 2), "tanh2": ((7, 13), "tanh", 1),
        "tanh2_o2": ((7, 13), "tanh", 2), "relu1": ((9,), "relu", 1), "relu2_o2": ((7, 13), "relu", 2)}


def _old_mlp(ct, R, layers, act, g, seed=7, size=0.25):
    lay = [(W.astype(np.float64), b.astype(np.float64)) for W, b in
           zip(_perturbed([W for W, _ in layers], seed, size), _perturbed([b for _, b in layers], seed + 1, size))]
    gt = torch.as_tensor(g)
    z = _torch_z(R, [(torch.as_tensor(W), torch.as_tensor(b)) for W, b in lay], act, gt).numpy()
    return log_pi(z, R["labels"]).astype(np.float32)


@pytest.mark.parametrize("name", list(NETS))
def test_mlp_restatement_is_the_gradient_of_the_clipped_surrogate(mini, name):
    ct, runs, w, A, g = mini
    hidden, act, n_out = NETS[name]
    layers = E.net(ct, hidden, n_out, seed=5)
    R = runs[True]
    old = _old_mlp(ct, R, layers, act, g).astype(np.float64)
    ref = surrogate_mlp_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, A, old, CLIP, BETA, layers, act, g, E.G)
    lt = [(torch.tensor(W.astype(np.float64), requires_grad=True), torch.tensor(b.astype(np.float64), requires_grad=True))
          for W, b in layers]
    total, L, kl, H = _torch_objective(R, w, A, old, CLIP, BETA, lt, act, g, E.G)
    total.backward()
    for (dW, db), (Wt, bt) in zip(ref["layers"], lt):
        assert _rel(dW, Wt.grad.numpy()) <= 1e-10 and _rel(db, bt.grad.numpy()) <= 1e-10, name
    np.testing.assert_allclose(ref["L"], L, rtol=1e-9, atol=1e-9)  # two fp64 log-sigmoids, their difference times rho
    np.testing.assert_allclose(ref["kl"], kl, rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(ref["H"], H, rtol=1e-12, atol=1e-12)
    assert all((bW >= 0).all() and (bb >= 0).all() for bW, bb in ref["bound"])
    _clips_both_ways(ref, A, name)


def test_without_old_log_prob_and_entropy_it_is_the_weighted_imitation_restatement(mini):
    """old_log_prob=None, beta=0: rho = 1, nothing clips, and the gradient is imitation_gradient(day_weight=A)'s"""
    ct, runs, w, A, g = mini
    R = runs[True]
    W, b = E.linear_params(ct)
    got = surrogate_linear_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, A, None, CLIP, 0.0, W, b, g, E.G)
    want = weighted_imitation_linear_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, A, W, b, g, E.G)
    np.testing.assert_allclose(got["weight"], want["weight"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(got["bias"], want["bias"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(got["L"], np.where(R["valid"] & ~R["forced"], A, 0.0).sum(axis=0), rtol=1e-12, atol=1e-14)
    layers = E.net(ct, (7, 13), 2, seed=5)
    gotm = surrogate_mlp_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, A, None, CLIP, 0.0, layers, "tanh", g, E.G)
    wantm = weighted_imitation_mlp_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, A, layers, "tanh", g, E.G)
    for (dW, db), (rW, rb) in zip(gotm["layers"], wantm["layers"]):
        np.testing.assert_allclose(dW, rW, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(db, rb, rtol=1e-12, atol=1e-14)
    assert (gotm["clipped"] == 0).all() and (gotm["kl"] == 0).all()


def _moved(ref, mut):
    return bool((np.abs(np.concatenate([mut["weight"], mut["bias"][:, None]], axis=1)
                        - np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1)) > ref["bound"]).any())


def _moved_mlp(ref, mut):
    return any((np.abs(m - r) > bd).any() for (mW, mb), (rW, rb), (bW, bb) in zip(mut["layers"], ref["layers"], ref["bound"])
               for m, r, bd in ((mW, rW, bW), (mb, rb, bb)))


def test_mutants_move_the_gradient_beyond_the_bound(mini):
    """clipping on rho alone whatever the sign of A, the clip test with the signs of A swapped, rho dropped from the
    coefficient, the entropy term's sign flipped: each moves some component by more than the bound the GPU tests hold
    the kernels to (ambiguous days included in that bound)."""
    ct, runs, w, A, g = mini
    R = runs[True]
    W, b = E.linear_params(ct)
    layers = E.net(ct, (7, 13), 1, seed=5)
    for moved, fn, par, old in ((_moved, surrogate_linear_fp64, (W, b), _old_linear(ct, R, g)),
                                (_moved_mlp, surrogate_mlp_fp64, (layers, "tanh"), _old_mlp(ct, R, layers, "tanh", g))):
        args = (R["obs"], R["labels"], R["valid"], R["forced"], w, A, old.astype(np.float64), CLIP, BETA)
        ref = fn(*args, *par, g, E.G)
        assert ref["ambiguous_share"] <= AMBIGUOUS_CAP
        for mutant in ("clip_rho_only", "swap_sign", "no_rho", "entropy_sign"):
            assert moved(ref, fn(*args, *par, g, E.G, mutant=mutant)), (fn.__name__, mutant)


def test_entropy_and_clip_edges_of_the_restatement():
    z = np.array([0.0, 800.0, -800.0, 2.0])
    H = entropy(z)
    assert abs(H[0] - np.log(2)) < 1e-15 and H[1] == 0.0 and H[2] == 0.0
    h = 1e-6
    np.testing.assert_allclose((entropy(z[3] + h) - entropy(z[3] - h)) / (2 * h),
                               -z[3] * np.exp(log_pi(z[3], 1)) * np.exp(log_pi(z[3], 0)), rtol=1e-8)
    # clip = 0 and a clip so large that nothing clips, on one env-day per sign of A
    obs, lab, ones = np.ones((1, 2, 1)), np.ones((1, 2), bool), np.ones((1, 2), bool)
    A, old = np.array([[1.0, -1.0]]), np.array([[-1.0, -0.2]])  # lp = log sigmoid(0.5) = -0.474: rho > 1 and rho < 1
    for clip, clipped in ((0.0, 2), (100.0, 0)):
        r = surrogate_linear_fp64(obs, lab, ones, ~ones, None, A, old, clip, 0.0, np.array([[0.5]]), np.array([0.0]), None, 1)
        assert r["clipped"].sum() == clipped and (r["weight"] == 0).all() == (clipped == 2)


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


def test_header_and_ffi_signatures_agree(lib):
    """the argument count and the kind of every argument of the new entry points, header against _ffi's argtypes"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "w2a.h")).read()
    for name in NEW:
        i = re.search(rf"^(?:size_t|int) {name}\(", text, re.M).end() - len(name) - 2
        args = [a.strip() for a in text[text.index("(", i) + 1:text.index(");", i)].replace("\n", " ").split(",")]
        kinds = ["p" if "*" in a else {"int32_t": "i32", "int64_t": "i64", "size_t": "sz", "double": "f64"}[a.split()[0]]
                 for a in args]
        have = ["p" if (t is C.c_void_p or hasattr(t, "_type_") and not isinstance(t._type_, str)) else
                {C.c_int32: "i32", C.c_int64: "i64", C.c_size_t: "sz", C.c_double: "f64"}[t]
                for t in getattr(lib, name).argtypes]
        assert kinds == have, (name, kinds, have)
        ret = text[:i].rsplit("\n", 1)[-1].strip()
        assert (getattr(lib, name).restype is C.c_size_t) == (ret == "size_t") and ret in ("size_t", "int"), name


def _err(lib):
    return lib.w2a_last_error().decode()


def test_bad_arguments_are_refused_on_the_host(lib):
    """NULL and bad arguments return -1 (W2A_ERR_ARG) with a message naming the entry point, in the order of the
    weighted imitation calls; nothing is launched (there is no device here, and the handle is NULL throughout). The fake
    pointers are never dereferenced: the handle is checked before anything reads them."""
    P = 4096  # a non-NULL, 256-B aligned address that is never read
    names = ("alert_mask", "mask_words", "env_weight", "advantage", "advantage_days", "old_log_prob", "old_log_prob_days",
             "clip", "entropy_coef", "n_steps", "obs", "grad", "surrogate", "clipped_days", "approx_kl", "entropy", "days",
             "log_prob")
    ok = dict(zip(names, (P, 5, None, P, 3, None, 0, 0.2, 0.0, 3, P, P, P, P, P, P, P, None)))

    def call(fn, pol, tail, **kw):
        a = dict(ok)
        a.update(kw)
        return fn(None, pol, *(a[k] for k in names), *tail)

    def common(fn, pol, tail, who):
        assert call(fn, pol, tail, n_steps=0) == -1 and "n_steps" in _err(lib)
        assert call(fn, pol, tail, alert_mask=None) == -1 and "alert_mask" in _err(lib)
        assert call(fn, pol, tail, obs=None) == -1 and "NULL obs" in _err(lib)
        for k in ("grad", "surrogate", "clipped_days", "approx_kl", "entropy", "days"):
            assert call(fn, pol, tail, **{k: None}) == -1 and "NULL grad, surrogate" in _err(lib), k
        assert call(fn, pol, tail, advantage=None) == -1 and "NULL advantage" in _err(lib)
        assert call(fn, pol, tail, advantage_days=2) == -1 and "advantage holds fewer" in _err(lib)
        assert call(fn, pol, tail, old_log_prob=P, old_log_prob_days=2) == -1 and "old_log_prob holds fewer" in _err(lib)
        for bad in (-0.1, float("nan"), float("inf")):
            assert call(fn, pol, tail, clip=bad) == -1 and "clip" in _err(lib)
        for bad in (float("nan"), float("-inf")):
            assert call(fn, pol, tail, entropy_coef=bad) == -1 and "entropy_coef" in _err(lib)
        # an output is looked at before the advantage, the advantage before the handle
        assert call(fn, pol, tail, days=None, advantage=None) == -1 and "NULL grad" in _err(lib)
        assert call(fn, pol, tail, old_log_prob=P, old_log_prob_days=3, log_prob=P, clip=0.0, entropy_coef=-1.0) == -1
        assert "NULL handle" in _err(lib) and _err(lib).startswith(who + ":")

    lp = _ffi.LinearPolicy()
    lin = lib.w2a_surrogate_gradient_linear
    assert call(lin, None, (None,)) == -1 and "NULL policy" in _err(lib)
    lp.weight, lp.bias, lp.n_groups = P, P, 1
    common(lin, C.byref(lp), (None,), "w2a_surrogate_gradient_linear")
    lp.weight = P + 4
    assert call(lin, C.byref(lp), (None,)) == -1 and "16-B aligned" in _err(lib)
    lp.weight, lp.require_budget = P, 2
    assert call(lin, C.byref(lp), (None,)) == -1 and "require_budget" in _err(lib)

    mp = _ffi.MlpPolicy()
    mlp = lib.w2a_surrogate_gradient_mlp
    tail = (P, 1 << 20, None)
    assert call(mlp, None, tail) == -1 and "NULL policy" in _err(lib)
    mp.params, mp.n_groups, mp.n_layers, mp.width = P, 1, 2, 48
    assert call(mlp, C.byref(mp), tail) == -1 and "width" in _err(lib)
    mp.width = 64
    common(mlp, C.byref(mp), tail, "w2a_surrogate_gradient_mlp")
    assert call(mlp, C.byref(mp), (None, 1 << 20, None)) == -1 and "NULL workspace" in _err(lib)
    assert call(mlp, C.byref(mp), (P + 64, 1 << 20, None)) == -1 and "256-B aligned" in _err(lib)
    assert call(mlp, C.byref(mp), (None, 1 << 20, None), advantage=None) == -1 and "NULL workspace" in _err(lib)
    size = lib.w2a_surrogate_gradient_mlp_workspace_bytes
    assert size(0, 10, 1, 16, 1) == 0 and size(100, 10, 1, 48, 1) == 0 and size(100, 10, 1, 16, 3) == 0
    for shape in ((100, 10, 1, 16, 1), (70_000, 153, 5, 64, 2)):
        assert size(*shape) == lib.w2a_imitation_gradient_mlp_workspace_bytes(*shape) > 0 and size(*shape) % 256 == 0


def test_python_argument_checks():
    """policy.check_surrogate_args: everything surrogate_gradient() refuses beyond imitation_gradient()'s arguments"""
    n, cpu = 6, torch.device("cpu")
    adv, old = np.ones((7, n)), -np.ones((5, n))
    a, o, clip, beta = policy.check_surrogate_args(adv, old, 0.2, 0, 5, n, cpu)
    assert a.dtype == torch.float32 and a.shape == (7, n) and a.is_contiguous() and o.shape == (5, n)
    assert clip == 0.2 and isinstance(beta, float) and beta == 0.0
    assert policy.check_surrogate_args(torch.as_tensor(adv), None, 0, -0.5, 5, n, cpu)[1] is None
    nan, pos = adv.copy(), old.copy()
    nan[4, 2], pos[1, 1] = np.nan, 1e-3
    bad = [dict(advantage=None), dict(advantage=np.ones((4, n))), dict(advantage=np.ones((5, n + 1))),
           dict(advantage=np.ones(n)), dict(advantage=np.ones((5, n), np.int64)), dict(advantage=nan),
           dict(advantage=adv * np.inf), dict(advantage=np.full((5, n), 1e39)), dict(old_log_prob=-np.ones((4, n))),
           dict(old_log_prob=-np.ones((5, n - 1))), dict(old_log_prob=pos), dict(old_log_prob=-nan),
           dict(old_log_prob=-np.ones((5, n), np.int32)), dict(clip=-0.1), dict(clip=np.nan), dict(clip=np.inf),
           dict(clip="0.2"), dict(clip=None), dict(clip=True), dict(entropy_coef=np.nan), dict(entropy_coef=-np.inf),
           dict(entropy_coef=None)]
    for kw in bad:
        k = dict(advantage=adv, old_log_prob=old, clip=0.2, entropy_coef=0.0)
        k.update(kw)
        with pytest.raises(ValueError, match=r"surrogate_gradient\(\): " + next(iter(kw))):
            policy.check_surrogate_args(k["advantage"], k["old_log_prob"], k["clip"], k["entropy_coef"], 5, n, cpu)
    # the shared checks name this caller
    with pytest.raises(ValueError, match="surrogate_gradient"):
        policy.check_imitation_args("never", np.zeros((n, 40), bool), None, None, n, 40, cpu, who="surrogate_gradient()")
    with pytest.raises(ValueError, match=r"imitation_gradient\(\): day_weight"):  # the defaults are what they were
        policy.check_day_weight(np.ones((4, n)), 5, n, cpu)
