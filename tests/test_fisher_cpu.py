"""fisher_vector_product() without a device: the fp64 restatement (tests/fisher_restatement.py) against fp64 torch
autograd, the argument checks of policy.check_fisher_args, what the three new exports refuse before they look at the
handle (in the manner of tests/test_policy_entry_refusals_cpu.py) and the ABI."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fisher_restatement import AMBIGUOUS_CAP, fisher_linear_fp64, fisher_mlp_fp64  # noqa: E402

from weather2alert_amd import _ffi, build, policy  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S, N_OBS, G = 40, 12, 9, 3
REL = 1e-10  # both sides are fp64 and exact in exact arithmetic: anything larger is a wrong formula


def _rows(seed=0):
    """random rows, a schedule, ragged valid days, forced days, weights with zeros and both signs, groups 0 and 2 of 3"""
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((S, N, N_OBS))
    labels = rng.random((S, N)) < 0.4
    length = rng.integers(0, S + 1, N)  # an env finished on entry (0 days) and envs that run the whole call
    length[:3] = (0, S, 1)
    valid = np.arange(S)[:, None] < length[None, :]
    forced = (rng.random((S, N)) < 0.2) & valid
    w = rng.standard_normal(N)
    w[::7] = 0.0
    g = np.array([0, 2])[np.arange(N) % 2]
    assert forced.any() and (valid & ~forced).any()
    return obs, labels, valid, forced, w, g


def _dyadic(rng, shape, scale=1.0):
    """f32-exact values with few mantissa bits: row1 - row0 of a two-row output is then exact in f32, so the host's one
    rounding of the fold changes nothing and torch's unrounded fold is the same number"""
    return np.round(rng.standard_normal(shape) * scale * 256.0) / 256.0


def _net(rng, hidden, n_out, scale):
    dims = [N_OBS] + list(hidden)
    layers = [(rng.standard_normal((G, dims[i + 1], dims[i])).astype(np.float32) * np.float32(scale / np.sqrt(dims[i])),
               (rng.standard_normal((G, dims[i + 1])) * 0.3).astype(np.float32)) for i in range(len(hidden))]
    layers.append((_dyadic(rng, (G, n_out, dims[-1]), scale / np.sqrt(dims[-1])).astype(np.float32),
                   _dyadic(rng, (G, n_out), 0.3).astype(np.float32)))
    return layers


def test_linear_restatement_is_minus_the_hessian_vector_product_of_the_log_likelihood():
    """F v = -H v of the restated log-likelihood (the logistic Hessian does not depend on the labels), per group as the
    mean over its envs; <v, F v> = group_quadratic."""
    obs, labels, valid, forced, w, g = _rows()
    rng = np.random.default_rng(1)
    W, b = rng.standard_normal((G, N_OBS)) * 0.5, rng.standard_normal(G) * 0.5
    vW, vb = rng.standard_normal((G, N_OBS)), rng.standard_normal(G)
    ref = fisher_linear_fp64(obs, labels, valid, forced, w, W, b, vW, vb, g, G)
    m = torch.as_tensor(valid & ~forced)
    o, a = torch.as_tensor(obs), torch.as_tensor(labels).double()
    gt, wt = torch.as_tensor(g), torch.as_tensor(w)
    cnt = torch.as_tensor(np.maximum(np.bincount(g, minlength=G), 1)).double()

    def loglik(Wt, bt):
        z = torch.einsum("snj,nj->sn", o, Wt[gt]) + bt[gt][None, :]
        ll = -torch.nn.functional.softplus(torch.where(a.bool(), -z, z))
        return ((ll * m).sum(0) * wt / cnt[gt]).sum()  # the sum over groups of each group's weighted mean

    _, (hW, hb) = torch.autograd.functional.hvp(loglik, (torch.as_tensor(W), torch.as_tensor(b)),
                                                (torch.as_tensor(vW), torch.as_tensor(vb)))
    have = np.bincount(g, minlength=G) > 0
    assert np.isnan(ref["weight"][~have]).all() and np.isnan(ref["bias"][~have]).all() and (~have).any()
    scale = max(np.abs(ref["weight"][have]).max(), np.abs(ref["bias"][have]).max())
    assert np.abs(ref["weight"][have] + hW.numpy()[have]).max() <= REL * scale
    assert np.abs(ref["bias"][have] + hb.numpy()[have]).max() <= REL * scale
    quad = (vW * ref["weight"]).sum(axis=1) + vb * ref["bias"]
    assert np.abs(quad - ref["group_quadratic"])[have].max() <= REL * np.abs(ref["group_quadratic"][have]).max()
    assert np.isnan(ref["group_quadratic"][~have]).all()
    np.testing.assert_array_equal(ref["days"], (valid & ~forced).sum(axis=0))
    assert (ref["bound"][have] > 0).all() and (ref["quadratic_bound"] >= 0).all()


MLP_CASES = {"tanh_h7": ((7,), "tanh", 1), "relu_h11_o2": ((11,), "relu", 2), "tanh_h7x5_o2": ((7, 5), "tanh", 2),
             "relu_h6x9": ((6, 9), "relu", 1)}


def _torch_fv(layers, vector, activation, obs, m, w, g):
    """J^T diag(w p q) J v per group from torch.autograd.functional.jvp / vjp, the mean over the group's envs"""
    act = torch.tanh if activation == "tanh" else torch.relu
    out = [(np.full(W.shape, np.nan), np.full(b.shape, np.nan)) for W, b in layers]
    quad = np.full(G, np.nan)
    for k in range(G):
        sel = g == k
        if not sel.any():
            continue
        x = torch.as_tensor(obs[:, sel])
        theta = tuple(torch.as_tensor(t[k]).double() for pair in layers for t in pair)
        vk = tuple(torch.as_tensor(t[k]).double() for pair in vector for t in pair)

        def logit(*th):
            h = x
            for i in range(0, len(th) - 2, 2):
                h = act(torch.einsum("snj,uj->snu", h, th[i]) + th[i + 1])
            zz = torch.einsum("snj,uj->snu", h, th[-2]) + th[-1]
            return zz[..., 0] if zz.shape[-1] == 1 else zz[..., 1] - zz[..., 0]

        z, u = torch.autograd.functional.jvp(logit, theta, vk)
        p = torch.sigmoid(z)
        pq = p * (1.0 - p) * torch.as_tensor(m[:, sel])
        c = pq * u * torch.as_tensor(w[sel])[None, :] / int(sel.sum())
        _, fv = torch.autograd.functional.vjp(logit, theta, c)
        for i in range(len(layers)):
            out[i][0][k], out[i][1][k] = fv[2 * i].numpy(), fv[2 * i + 1].numpy()
        quad[k] = float(((pq * u * u).sum(0) * torch.as_tensor(w[sel])).mean())
    return out, quad


@pytest.mark.parametrize("case", list(MLP_CASES))
def test_mlp_restatement_is_jt_diag_wpq_j_v(case):
    """tanh and ReLU, one and two hidden layers, n_out 1 and 2: the restated product and quadratic form against
    J^T diag(w p q) J v built from torch's jvp and vjp in fp64"""
    hidden, activation, n_out = MLP_CASES[case]
    obs, labels, valid, forced, w, g = _rows(seed=2)
    rng = np.random.default_rng(len(hidden) * 10 + hidden[0])
    layers, vector = _net(rng, hidden, n_out, 1.0), _net(rng, hidden, n_out, 1.0)
    ref = fisher_mlp_fp64(obs, labels, valid, forced, w, layers, vector, activation, g, G)
    assert ref["near_kink"] <= AMBIGUOUS_CAP
    obs0 = np.where(valid[:, :, None], obs, 0.0)
    want, quad = _torch_fv(layers, vector, activation, obs0, valid & ~forced, w, g)
    have = np.bincount(g, minlength=G) > 0
    scale = max(np.abs(x[have]).max() for pair in ref["layers"] for x in pair)
    assert scale > 0
    for (rW, rb), (tW, tb), (lW, lb) in zip(ref["layers"], want, layers):
        assert rW.shape == lW.shape and rb.shape == lb.shape
        assert np.isnan(rW[~have]).all() and np.isnan(rb[~have]).all()
        assert np.abs(rW - tW)[have].max() <= REL * scale and np.abs(rb - tb)[have].max() <= REL * scale
    assert np.abs(quad - ref["group_quadratic"])[have].max() <= REL * np.abs(quad[have]).max()
    inner = sum((np.asarray(V, np.float64) * rW).sum(axis=(1, 2)) + (np.asarray(vb, np.float64) * rb).sum(axis=1)
                for (V, vb), (rW, rb) in zip(vector, ref["layers"]))
    assert np.abs(inner - quad)[have].max() <= REL * np.abs(quad[have]).max()
    for bW, bb in ref["bound"]:
        assert (bW[have] >= 0).all() and (bb[have] >= 0).all()


def test_the_restatement_tells_a_wrong_estimator_apart():
    """every mutant leaves its own bound by orders of magnitude: the bound is no blanket"""
    obs, labels, valid, forced, w, g = _rows(seed=3)
    rng = np.random.default_rng(4)
    W, b = rng.standard_normal((G, N_OBS)) * 0.5, rng.standard_normal(G) * 0.5
    vW, vb = rng.standard_normal((G, N_OBS)), rng.standard_normal(G)
    ref = fisher_linear_fp64(obs, labels, valid, forced, w, W, b, vW, vb, g, G)
    have = np.bincount(g, minlength=G) > 0
    for mutant in ("no_q", "no_bias"):
        bad = fisher_linear_fp64(obs, labels, valid, forced, w, W, b, vW, vb, g, G, mutant=mutant)
        assert (np.abs(bad["weight"] - ref["weight"])[have] > 1e3 * ref["bound"][have][:, :-1]).any(), mutant
    bad = fisher_linear_fp64(obs, labels, valid, forced, w, W, b, vW, vb, g, G, mutant="quad_weighted")
    assert (np.abs(bad["quadratic"] - ref["quadratic"]) > 1e3 * ref["quadratic_bound"]).any()
    layers, vector = _net(rng, (7, 5), 1, 1.0), _net(rng, (7, 5), 1, 1.0)
    ref = fisher_mlp_fp64(obs, labels, valid, forced, w, layers, vector, "tanh", g, G)
    for mutant in ("no_q", "no_bias", "dact_pre"):
        bad = fisher_mlp_fp64(obs, labels, valid, forced, w, layers, vector, "tanh", g, G, mutant=mutant)
        assert (np.abs(bad["layers"][0][0] - ref["layers"][0][0])[have] > 1e3 * ref["bound"][0][0][have]).any(), mutant


# ---- check_fisher_args ------------------------------------------------------------------------------------------------
OBS_SLOT = list(range(N_OBS))


def _lin_pol(G_=2):
    rng = np.random.default_rng(5)
    pol = dict(kind="linear", weight=rng.standard_normal((G_, N_OBS)).astype(np.float32),
               bias=rng.standard_normal(G_).astype(np.float32))
    if G_ > 1:
        pol["group"] = np.arange(10) % G_
    return policy.check_linear_policy(pol, N_OBS, 10, OBS_SLOT, "cpu")


def _mlp_pol(G_=2, n_out=2):
    rng = np.random.default_rng(6)
    layers = [(rng.standard_normal((G_, 7, N_OBS)).astype(np.float32), rng.standard_normal((G_, 7)).astype(np.float32)),
              (rng.standard_normal((G_, 13, 7)).astype(np.float32), rng.standard_normal((G_, 13)).astype(np.float32)),
              (rng.standard_normal((G_, n_out, 13)).astype(np.float32), rng.standard_normal((G_, n_out)).astype(np.float32))]
    pol = dict(kind="mlp", layers=layers, group=np.arange(10) % G_) if G_ > 1 else dict(kind="mlp", layers=layers)
    return policy.check_mlp_policy(pol, N_OBS, 10, OBS_SLOT, "cpu"), layers


def test_check_fisher_args_packs_the_vector_as_the_policy_is_packed():
    lin = _lin_pol()
    v = {"weight": np.arange(2 * N_OBS, dtype=np.float32).reshape(2, N_OBS), "bias": np.array([3.0, 4.0], np.float32)}
    vw, vb = policy.check_fisher_args("linear", v, lin, N_OBS, OBS_SLOT, "cpu")
    assert vw.shape == (2, 32) and vw.dtype == torch.float32 and torch.equal(vw[:, :N_OBS], torch.as_tensor(v["weight"]))
    assert bool((vw[:, N_OBS:] == 0).all()) and torch.equal(vb, torch.as_tensor(v["bias"]))
    mlp, layers = _mlp_pol()
    P = policy.check_fisher_args("mlp", {"layers": layers}, mlp, N_OBS, OBS_SLOT, "cpu")
    assert torch.equal(P, mlp.params)  # the policy's own parameters as the vector: the same packing, fold and padding
    # <pack(v), block> = <v, unpack(block)>: the product comes back through the adjoint of the packing
    block = torch.as_tensor(np.random.default_rng(7).standard_normal(tuple(P.shape))).float()
    back = policy.unpack_mlp_grad(block, OBS_SLOT, N_OBS, mlp.hidden, mlp.n_out)
    inner = sum(float((torch.as_tensor(V).double() * dW.double()).sum() + (torch.as_tensor(vb_).double() * db.double()).sum())
                for (V, vb_), (dW, db) in zip(layers, back))
    assert abs(inner - float((P.double() * block.double()).sum())) <= 1e-4 * float((P.abs() * block.abs()).sum())
    one, layers1 = _mlp_pol(G_=1, n_out=1)
    flat = {"layers": [(W[0], b[0]) for W, b in layers1]}  # G == 1: the leading axis may be left out
    assert torch.equal(policy.check_fisher_args("mlp", flat, one, N_OBS, OBS_SLOT, "cpu"), one.params)


def test_check_fisher_args_refusals():
    lin, (mlp, layers) = _lin_pol(), _mlp_pol()
    vw, vb = np.zeros((2, N_OBS), np.float32), np.zeros(2, np.float32)
    nan_w = vw.copy()
    nan_w[1, 3] = np.nan
    bad_linear = [None, {"layers": layers}, {"weight": vw}, {"weight": vw[:, :-1], "bias": vb},
                  {"weight": vw[:1], "bias": vb[:1]},  # wrong G
                  {"weight": vw, "bias": np.zeros(3, np.float32)}, {"weight": nan_w, "bias": vb},
                  {"weight": vw, "bias": np.array([0.0, np.inf], np.float32)},
                  {"weight": vw.astype(np.int32), "bias": vb}]
    for v in bad_linear:
        with pytest.raises(ValueError, match=r"fisher_vector_product\(\)"):
            policy.check_fisher_args("linear", v, lin, N_OBS, OBS_SLOT, "cpu")

    def swap(i, j, x):
        out = [list(p) for p in layers]
        out[i][j] = x
        return {"layers": [tuple(p) for p in out]}

    inf_b = layers[1][1].copy()
    inf_b[0, 2] = np.inf
    huge = layers[2][0].copy()
    huge[0, 0, 0], huge[0, 1, 0] = -3e38, 3e38  # finite rows whose fold row1 - row0 is not finite as float32
    bad_mlp = [None, {"weight": vw, "bias": vb},  # the wrong kind's vector
               {"layers": layers[:2]}, {"layers": [layers[0], layers[1], layers[2][0]]},
               swap(0, 0, layers[0][0][:, :, :-1]), swap(0, 1, layers[0][1][:, :-1]),  # wrong shapes, layer by layer
               swap(1, 0, layers[1][0][:, :-1]), swap(1, 0, np.swapaxes(layers[1][0], 1, 2)),
               swap(2, 0, layers[2][0][:, :1]), swap(2, 1, layers[2][1][:, :1]),  # one output row for a two-row policy
               {"layers": [(W[:1], b[:1]) for W, b in layers]},  # wrong G
               {"layers": [(W[0], b[0]) for W, b in layers]},
               swap(1, 1, inf_b), swap(2, 0, huge), swap(0, 0, layers[0][0].astype(np.int64))]
    for v in bad_mlp:
        with pytest.raises(ValueError, match=r"fisher_vector_product\(\)"):
            policy.check_fisher_args("mlp", v, mlp, N_OBS, OBS_SLOT, "cpu")


# ---- the exports without a handle ---------------------------------------------------------------------------------------
P = 4096  # a non-NULL, 256-B aligned address that is never read
OBS = "NULL obs (the rows the agent holds are the first day's input)"


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


def _family(kind):
    if kind == "linear":
        names = ("vec_weight", "vec_bias", "alert_mask", "mask_words", "env_weight", "n_steps", "obs", "fv", "quadratic",
                 "days", "stream", "allowed_days", "allowed_words")
        checks = [({"policy": None}, "NULL policy"), ({"n_steps": 0}, "n_steps must be positive"),
                  ({"p.weight": None}, "NULL weight or bias"), ({"p.bias": None}, "NULL weight or bias"),
                  ({"p.n_groups": 0}, "n_groups must be positive"), ({"p.sample": 2}, "sample must be 0 or 1"),
                  ({"p.require_budget": 2}, "require_budget must be 0 or 1"),
                  ({"p.weight": P + 4}, "weight must be 16-B aligned"),
                  ({"vec_weight": None}, "NULL vec_weight or vec_bias"), ({"vec_bias": None}, "NULL vec_weight or vec_bias"),
                  ({"vec_weight": P + 4}, "vec_weight must be 16-B aligned")]
    else:
        names = ("vector", "alert_mask", "mask_words", "env_weight", "n_steps", "obs", "fv", "quadratic", "days",
                 "workspace", "workspace_bytes", "stream", "allowed_days", "allowed_words")
        checks = [({"policy": None}, "NULL policy"), ({"n_steps": 0}, "n_steps must be positive"),
                  ({"p.params": None}, "NULL params"), ({"p.n_groups": -1}, "n_groups must be positive"),
                  ({"p.n_layers": 3}, "n_layers must be 1 or 2"), ({"p.width": 48}, "width must be 16, 32 or 64"),
                  ({"p.activation": 2}, "activation must be W2A_MLP_TANH or W2A_MLP_RELU"),
                  ({"p.sample": 2}, "sample must be 0 or 1"), ({"p.require_budget": 2}, "require_budget must be 0 or 1"),
                  ({"p.params": P + 16 + 8}, "params must be 16-B aligned"),
                  ({"vector": None}, "NULL vector"), ({"vector": P + 8}, "vector must be 16-B aligned")]
    checks += [({"alert_mask": None}, "NULL alert_mask (the schedule to follow)"), ({"obs": None}, OBS)]
    checks += [({k: None}, "NULL fv, quadratic or days") for k in ("fv", "quadratic", "days")]
    if kind == "mlp":
        checks += [({"workspace": None}, "NULL workspace"), ({"workspace": P + 64}, "workspace must be 256-B aligned")]
    ok = dict(vec_weight=P, vec_bias=P, vector=P, alert_mask=P, mask_words=0, env_weight=None, n_steps=3, obs=P, fv=P,
              quadratic=P, days=P, workspace=P, workspace_bytes=1 << 20, stream=None, allowed_days=None, allowed_words=0)
    return names, ok, checks


def _call(lib, name, kind, names, ok, bad):
    if kind == "linear":
        pol = _ffi.LinearPolicy(weight=P, bias=P, group=None, n_groups=1, sample=1, require_budget=0, seed=0)
    else:
        pol = _ffi.MlpPolicy(params=P, group=None, order=None, n_groups=1, n_layers=2, width=64, activation=0, sample=1,
                             require_budget=0, seed=0)
    a = dict(ok, policy=C.byref(pol))
    for k, v in bad.items():
        if k.startswith("p."):
            setattr(pol, k[2:], v)
        else:
            a[k] = v
    rc = getattr(lib, name)(None, a["policy"], *(a[k] for k in names))
    return rc, lib.w2a_last_error().decode()


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_refusals_without_a_handle_and_their_order(lib, kind):
    """return code and full error text of every check that comes before the handle is read; with two bad arguments the
    earlier check reports; the gate is nullable and looked at after the handle"""
    name = f"w2a_fisher_vector_product_{kind}"
    names, ok, checks = _family(kind)
    assert len(names) + 2 == len(getattr(lib, name).argtypes)
    assert _call(lib, name, kind, names, ok, {}) == (-1, f"{name}: NULL handle")
    assert _call(lib, name, kind, names, ok, {"allowed_days": P, "allowed_words": 0}) == (-1, f"{name}: NULL handle")
    for bad, text in checks:
        assert _call(lib, name, kind, names, ok, bad) == (-1, f"{name}: {text}"), bad
    pairs = 0
    for (bad1, text1), (bad2, _) in itertools.combinations(checks, 2):
        if bad1.keys() & bad2.keys():
            continue
        assert _call(lib, name, kind, names, ok, {**bad2, **bad1}) == (-1, f"{name}: {text1}"), (bad1, bad2)
        pairs += 1
    assert pairs > len(checks)


def test_workspace_size_is_the_policy_gradient_layout(lib):
    size = lib.w2a_fisher_vector_product_mlp_workspace_bytes
    for shape in ((100, 10, 1, 16, 1), (70_000, 153, 5, 64, 2), (1, 1, 3, 32, 2)):
        assert size(*shape) == lib.w2a_policy_gradient_mlp_workspace_bytes(*shape) > 0 and size(*shape) % 256 == 0
    for shape in ((0, 10, 1, 16, 1), (100, 0, 1, 16, 1), (100, 10, 0, 16, 1), (100, 10, 1, 48, 1), (100, 10, 1, 16, 3)):
        assert size(*shape) == 0


def test_abi_header_and_ffi_agree_on_the_new_names(lib):
    new = ["w2a_fisher_vector_product_linear", "w2a_fisher_vector_product_mlp",
           "w2a_fisher_vector_product_mlp_workspace_bytes"]
    header = open(os.path.join(ROOT, "include", "w2a.h")).read()
    declared = set(re.findall(r"\b(w2a_fisher_\w+)\s*\(", header))
    assert declared == set(new) == {s for s in _ffi.SYMBOLS if s.startswith("w2a_fisher_")}
    for s in new:
        assert getattr(lib, s).argtypes is not None
        proto = re.search(r"\b" + s + r"\s*\(([^;]*)\);", header).group(1)
        assert len(proto.split(",")) == len(getattr(lib, s).argtypes), s
    assert lib.w2a_abi_version() == _ffi.ABI_VERSION == 18
    assert re.search(r"W2A_ABI_VERSION\s*=?\s*18\b", header)
