"""rollout(mlp, policy_gradient=...) without a GPU: the fp64 restatement the GPU tests hold the kernels to
(tests/policy_gradient_mlp_restatement.py) is the gradient of the REINFORCE surrogate by torch autograd, its bound admits
the f32 evaluation and rejects three wrong gradients, the ReLU cases of the GPU tests are almost never near a kink,
every net of the instantiation matrix (tests/policy_gradient_mlp_cases.py) pads as listed and takes both actions in
every group, the block-layout helpers are adjoint to pack_mlp, and the C entry refuses bad arguments before any launch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from policy_gradient_mlp_cases import MATRIX, net as _case_net  # noqa: E402
from policy_gradient_mlp_restatement import policy_gradient_mlp_fp64  # noqa: E402
from policy_gradient_restatement import forced_days  # noqa: E402

from oracle import heatalert_oracle as O  # noqa: E402
from weather2alert_amd import _ffi, build, policy  # noqa: E402

# (hidden widths, activation, output rows): unpadded widths, one and two layers, a two-row output
NETS = {"tanh16": ((16,), "tanh", 1), "relu24x40": ((24, 40), "relu", 2), "tanh64x64": ((64, 64), "tanh", 2),
        "relu32x32": ((32, 32), "relu", 1), "tanh24": ((24,), "tanh", 2)}
# and the instantiation matrix of the GPU tests: padded widths under every (WIDTH, LAYERS) pair of the kernels
NETS.update({name: spec[1:] for name, spec in MATRIX.items()})


@pytest.fixture(scope="module")
def tabs():
    return E.make_tables()


@pytest.fixture(scope="module")
def recorded(tabs):
    """name -> the oracle's recorded trajectory of 200 envs under the sampled net, G = 5 interleaved groups, and the
    no-alert rewards (computed once, shared, left unchanged)"""
    tb = tabs["ragged"]
    ct, n = tb.ct, 200
    tup = E.host_tuples(tb, n)
    g = E.groups(n)
    uni = lambda t: O.devrng_policy_uniform_vec(E.POLICY_SEED, E.GID0 + np.arange(n), np.zeros(n, np.int64), t)  # noqa: E731
    out = {}
    V = tb.oracle()
    E.oracle_reset(V, tup)
    beta = np.zeros((ct.T, n))
    for s in range(ct.T):
        r, _, _, live = E.oracle_step(V, np.zeros(n, np.int64))
        beta[s] = np.where(live, r, 0.0)
    for name, (hidden, act, n_out) in NETS.items():
        layers = _case_net(ct, name, hidden, n_out)  # seed len(hidden) * 10 + hidden[0] unless the matrix names another
        E.oracle_reset(V, tup)
        R = E.oracle_record(V, lambda obs: E.mlp64(layers, act, obs, g), ct.T, (1e-5, 1e-5), uniform=uni, T=ct.T)
        forced = forced_days(True, tup["budget"], np.zeros(n, np.int64), R["alert"], R["valid"])
        out[name] = dict(R=R, layers=layers, act=act, g=g, beta=beta, forced=forced, ct=ct)
    return out


def _autograd(c, dtype, baseline, forced):
    """torch autograd of sum_e sum_s Q_s m_s log pi(a_s | o_s) / N_g: [(dW, db), ...] as numpy fp64"""
    R, g = c["R"], c["g"]
    valid = R["valid"]
    S = valid.shape[0]
    A = np.where(valid, R["reward"] - (0.0 if baseline is None else baseline), 0.0)
    Q = torch.as_tensor(np.cumsum(A[::-1], axis=0)[::-1].copy()).to(dtype)
    P = [(torch.tensor(np.asarray(W, np.float64)).to(dtype).requires_grad_(), torch.tensor(np.asarray(b, np.float64)).to(dtype).requires_grad_())
         for W, b in c["layers"]]
    gt = torch.as_tensor(g)
    h = torch.as_tensor(np.where(valid[:, :, None], R["obs"][:S], 0.0)).to(dtype)
    f = torch.tanh if c["act"] == "tanh" else torch.relu
    for W, b in P[:-1]:
        h = f(torch.einsum("snj,nuj->snu", h, W[gt]) + b[gt][None])
    Wo, bo = P[-1]
    if Wo.shape[1] == 2:  # the host's fold, rounded to f32 once (straight-through for the gradient)
        wo, b0 = Wo[:, 1] - Wo[:, 0], bo[:, 1] - bo[:, 0]
        wo = wo + (wo.detach().float().to(dtype) - wo.detach())
        b0 = b0 + (b0.detach().float().to(dtype) - b0.detach())
    else:
        wo, b0 = Wo[:, 0], bo[:, 0]
    z = (h * wo[gt][None]).sum(-1) + b0[gt][None]
    m = torch.as_tensor(valid & ~forced)
    lp = policy.action_log_prob(z, torch.as_tensor(R["action"]))
    cnt = torch.as_tensor(np.bincount(g, minlength=E.G).astype(np.float64)).to(dtype)
    (Q * torch.where(m, lp, torch.zeros_like(lp)) / cnt[gt][None]).sum().backward()
    return [(W.grad.double().numpy(), b.grad.double().numpy()) for W, b in P]


def _restate(c, baseline, forced, **kw):
    R = c["R"]
    return policy_gradient_mlp_fp64(R["obs"], R["action"], R["valid"], forced, R["reward"], baseline, c["layers"],
                                    c["act"], c["g"], E.G, **kw)


@pytest.mark.parametrize("name", list(NETS))
def test_restatement_is_the_gradient_of_the_surrogate(recorded, name):
    """(i) to 1e-10 relative, both baselines, with and without forced days"""
    c = recorded[name]
    assert c["R"]["alert"].any() and c["forced"][c["R"]["valid"]].any()
    for bl in (None, c["beta"]):
        for f in (np.zeros_like(c["forced"]), c["forced"]):
            ref = _restate(c, bl, f)
            want = _autograd(c, torch.float64, bl, f)
            scale = max(np.abs(x).max() for wb in want for x in wb)
            assert scale > 0
            for (dW, db), (aW, ab) in zip(ref["layers"], want):
                assert dW.shape == aW.shape and db.shape == ab.shape
                assert max(np.abs(dW - aW).max(), np.abs(db - ab).max()) <= 1e-10 * scale, name


def _outside(got, ref):
    return any((np.abs(x - r) > bd).any() for wb, rb, bb in zip(got, ref["layers"], ref["bound"])
               for x, r, bd in zip(wb, rb, bb))


@pytest.mark.parametrize("name", ["tanh64x64", "relu32x32", "relu24x40", "tanh16"])
def test_bound_admits_f32_and_rejects_wrong_gradients(recorded, name):
    """(ii) the estimator evaluated by torch in f32 lies inside the bound; Q shifted by one day, act' of the second layer
    omitted and W2 untransposed in the backward each leave it"""
    c = recorded[name]
    zero = np.zeros_like(c["forced"])
    ref = _restate(c, c["beta"], zero)
    f32 = _autograd(c, torch.float32, c["beta"], zero)
    worst = max(float((np.abs(x - r) / np.where(bd > 0, bd, 1.0)).max())
                for wb, rb, bb in zip(f32, ref["layers"], ref["bound"]) for x, r, bd in zip(wb, rb, bb))
    print(f"{name}: torch f32 vs restatement, max ratio to the bound {worst:.3e}")
    assert not _outside(f32, ref), (name, worst)
    share = max(float((sb / np.where(bd > 0, bd, 1.0)).max()) for s2, bb in zip(ref["bound_second"], ref["bound"])
                for sb, bd in zip(s2, bb))
    print(f"{name}: the second (absolute-error) term is at most {share:.3f} of a parameter's bound")
    assert _outside(_restate(c, c["beta"], zero, q_shift=1)["layers"], ref), "Q shifted by one day"
    hidden = NETS[name][0]
    if len(hidden) == 2:
        assert _outside(_restate(c, c["beta"], zero, drop_act2=True)["layers"], ref), "act' of layer 2 omitted"
        if hidden[0] == hidden[1]:
            assert _outside(_restate(c, c["beta"], zero, w2_untransposed=True)["layers"], ref), "W2 untransposed"


def test_f32_chain_emulation(recorded):
    """The accumulation term of the bound (16 S u per weight-gradient element, restatement docstring) against the
    kernel's exact f32 order replayed on the CPU for dW1 of the [16] tanh case, all 200 envs as one group: per 64-env
    tile and day 16 matrix-core steps of 4 envs, each a k-ordered fmaf chain into the tile's accumulator (two
    accumulators, even / odd steps, at width 16), the tile's sum then added in fp64. Terms: x (f32) times dh1 (fp64
    value rounded to f32 once). Measured against the exact sum of the same terms, relative to the sum of their
    magnitudes, in units of u."""
    c = recorded["tanh16"]
    R = c["R"]
    valid = R["valid"]
    S, N = valid.shape
    W1, b1 = (np.asarray(v, np.float64)[0] for v in c["layers"][0])
    wo = np.asarray(c["layers"][1][0], np.float64)[0, 0]
    x = np.where(valid[:, :, None], R["obs"][:S], 0.0).astype(np.float32)
    h = np.tanh(x.astype(np.float64) @ W1.T + b1)
    A = np.where(valid, R["reward"], 0.0)
    Q = np.cumsum(A[::-1], axis=0)[::-1]
    z = h @ wo + float(np.asarray(c["layers"][1][1])[0, 0])
    delta = np.where(valid, R["action"] - 1.0 / (1.0 + np.exp(-z)), 0.0)
    dh = ((delta * Q)[:, :, None] * wo[None, None, :] * (1.0 - h * h)).astype(np.float32)  # [S, N, 16]
    exact = np.einsum("snu,snj->uj", dh.astype(np.float64), x.astype(np.float64))
    mag = np.einsum("snu,snj->uj", np.abs(dh).astype(np.float64), np.abs(x).astype(np.float64))
    total = np.zeros_like(exact)
    for t0 in range(0, N, 64):
        acc = [np.zeros(exact.shape, np.float32), np.zeros(exact.shape, np.float32)]
        for s_ in range(S):
            for step in range(16):
                a = acc[step & 1]
                for e in range(t0 + 4 * step, min(t0 + 4 * step + 4, N)):
                    a = (a.astype(np.float64) + np.outer(dh[s_, e].astype(np.float64), x[s_, e].astype(np.float64))).astype(np.float32)
                acc[step & 1] = a
        total += (acc[0] + acc[1]).astype(np.float64)
    u = 2.0 ** -24
    worst = float((np.abs(total - exact) / np.where(mag > 0, mag, 1.0)).max() / u)
    print(f"f32 chain in the kernel's order, 64 x {S} terms per tile: max error {worst:.1f} u of the terms' magnitudes; "
          f"the bound allows {16 * S} u, the deterministic worst case is {64 * S} u")
    assert worst <= 0.1 * 16 * S


@pytest.mark.parametrize("name", ["relu24x40", "relu32x32"] + [k for k, v in MATRIX.items() if v[2] == "relu"])
def test_relu_cases_are_rarely_near_a_kink(recorded, name):
    """(iii) under 1 % of all unit-days, by the reference alone"""
    c = recorded[name]
    frac = _restate(c, None, np.zeros_like(c["forced"]))["near_kink"]
    print(f"{name}: near-kink unit-days {frac:.3e}")
    assert frac < 0.01


@pytest.mark.parametrize("name", list(MATRIX))
def test_matrix_nets_pad_as_listed_and_take_both_actions(recorded, name):
    """Every net of the instantiation matrix pads to the (WIDTH, LAYERS) pair it is listed under, and on the recorded
    batch its sampled policy takes both actions and issues alerts in every group: a gradient of all-zero deltas, or of
    one action only, would test little (the GPU tests' _twin_case asserts alerts on its own batch too)."""
    (width, n_layers), hidden, _, n_out = MATRIX[name]
    assert (policy.mlp_width(hidden), len(hidden)) == (width, n_layers)
    c = recorded[name]
    assert [tuple(W.shape[1:]) for W, _ in c["layers"]] == list(zip(list(hidden) + [n_out], [c["ct"].n_obs] + list(hidden)))
    R, g = c["R"], c["g"]
    free = R["valid"] & ~c["forced"]
    for k in range(E.G):
        a = R["action"][:, g == k][free[:, g == k]]
        assert (a == 1).any() and (a == 0).any(), (name, k)
        assert R["alert"][:, g == k].any(), (name, k)


@pytest.mark.parametrize("hidden,n_out", [((16,), 1), ((24, 40), 2), ((64, 64), 1), ((7,), 2), ((7, 13), 1), ((29, 9), 1),
                                          ((33,), 1), ((64,), 2)])
def test_unpack_is_the_adjoint_of_pack(tabs, hidden, n_out):
    """(iv) <pack(L), P> = <L, unpack(P)>, the two-row fold included (fp64 throughout: pack rounds to f32 last, so L is
    drawn on the f32 grid and the comparison made to that rounding)"""
    ct = tabs["slot27"].ct
    G = 3
    rng = np.random.default_rng(1)
    dims = [ct.n_obs] + list(hidden) + [n_out]
    L = [(torch.tensor(rng.integers(-8, 9, (G, dims[i + 1], dims[i])).astype(np.float64)),
          torch.tensor(rng.integers(-8, 9, (G, dims[i + 1])).astype(np.float64))) for i in range(len(dims) - 1)]
    packed, w, nl, G_ = policy.pack_mlp(L, ct.obs_slot, ct.n_obs)
    assert G_ == G and packed.shape == (G, policy.mlp_stride(w, nl))
    P = torch.tensor(rng.standard_normal(tuple(packed.shape)))
    U = policy.unpack_mlp_grad(P, ct.obs_slot, ct.n_obs, hidden, n_out)
    lhs = float((packed.double() * P).sum())
    rhs = float(sum((W * dW).sum() + (b * db).sum() for (W, b), (dW, db) in zip(L, U)))
    assert [tuple(dW.shape) for dW, _ in U] == [tuple(W.shape) for W, _ in L]
    assert abs(lhs - rhs) <= 1e-9 * max(1.0, abs(lhs))


def test_grad_to_module_writes_tensors_and_sign():
    """(v)"""
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Tanh(), torch.nn.Linear(7, 2))
    rng = np.random.default_rng(0)
    grad = {"layers": [(torch.tensor(rng.standard_normal((2, 7, 5)), dtype=torch.float32), torch.tensor(rng.standard_normal((2, 7)), dtype=torch.float32)),
                       (torch.tensor(rng.standard_normal((2, 2, 7)), dtype=torch.float32), torch.tensor(rng.standard_normal((2, 2)), dtype=torch.float32))]}
    policy.mlp_grad_to_module(net, grad, group=1)
    lins = [m for m in net if isinstance(m, torch.nn.Linear)]
    for m, (dW, db) in zip(lins, grad["layers"]):
        assert torch.equal(m.weight.grad, -dW[1]) and torch.equal(m.bias.grad, -db[1])
    policy.mlp_grad_to_module(net, grad, group=0, ascent=False)
    for m, (dW, db) in zip(lins, grad["layers"]):
        assert torch.equal(m.weight.grad, dW[0]) and torch.equal(m.bias.grad, db[0])
    w0 = lins[0].weight.detach().clone()
    policy.mlp_grad_to_module(net, grad, group=0, ascent=True)
    torch.optim.SGD(net.parameters(), lr=0.5).step()
    assert torch.allclose(lins[0].weight.detach(), w0 + 0.5 * grad["layers"][0][0][0])
    with pytest.raises(ValueError):
        policy.mlp_grad_to_module(torch.nn.Sequential(torch.nn.Linear(5, 1)), grad)


def test_check_policy_gradient_kinds():
    """(vi) rollout() passes kinds=("linear", "mlp"); the default still refuses mlp"""
    assert policy.check_policy_gradient(True, "mlp", True, kinds=("linear", "mlp")) == "no_alert"
    assert policy.check_policy_gradient("none", "linear", True, kinds=("linear", "mlp")) == "none"
    with pytest.raises(ValueError):
        policy.check_policy_gradient(True, "mlp", True)
    with pytest.raises(ValueError):
        policy.check_policy_gradient(True, "never", True, kinds=("linear", "mlp"))
    with pytest.raises(ValueError):
        policy.check_policy_gradient(True, "mlp", False, kinds=("linear", "mlp"))
    with pytest.raises(ValueError):
        policy.check_policy_gradient(True, "mlp", True, record=True, kinds=("linear", "mlp"))


def test_abi_symbols_and_refusals_without_a_gpu():
    """(vii) both symbols are exported and declared; bad arguments are refused on the host before the handle is used;
    the workspace holds at least pass 1's 9 B per env-day"""
    assert {"w2a_policy_gradient_mlp_workspace_bytes", "w2a_policy_gradient_mlp"} <= set(_ffi.SYMBOLS)
    build.build_lib()
    lib = _ffi.load(build_if_missing=False)
    wsb = lib.w2a_policy_gradient_mlp_workspace_bytes
    for n, S, G, w, nl in ((1000, 153, 1, 16, 1), (1 << 20, 153, 1024, 64, 2), (200, 17, 5, 32, 2)):
        assert wsb(n, S, G, w, nl) >= 9 * n * S
    assert wsb(0, 5, 1, 16, 1) == 0 and wsb(10, 0, 1, 16, 1) == 0 and wsb(10, 5, 1, 48, 1) == 0 and wsb(10, 5, 1, 16, 3) == 0
    mb = 1 << 20
    print("workspace at 1 048 576 envs x 153 days, [64, 64]: G = 1 %.0f MiB, G = 1024 %.0f MiB (pass 1's scratch %.0f MiB)"
          % (wsb(mb, 153, 1, 64, 2) / mb, wsb(mb, 153, 1024, 64, 2) / mb, 9 * 153))
    buf = (C.c_float * 64)()
    addr = (C.addressof(buf) + 255) & ~255

    def pol(**kw):
        p = _ffi.MlpPolicy()
        p.params, p.n_groups, p.n_layers, p.width, p.activation, p.sample, p.require_budget = addr, 1, 1, 16, 0, 1, 0
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    fn = lib.w2a_policy_gradient_mlp
    bad = [(None, 0, 3, addr, addr, addr), (pol(), 0, 0, addr, addr, addr), (pol(params=None), 0, 3, addr, addr, addr),
           (pol(n_groups=0), 0, 3, addr, addr, addr), (pol(n_layers=3), 0, 3, addr, addr, addr),
           (pol(width=48), 0, 3, addr, addr, addr), (pol(activation=2), 0, 3, addr, addr, addr),
           (pol(sample=0), 0, 3, addr, addr, addr), (pol(require_budget=2), 0, 3, addr, addr, addr),
           (pol(params=addr + 4), 0, 3, addr, addr, addr), (pol(), 2, 3, addr, addr, addr), (pol(), 0, 3, None, addr, addr),
           (pol(), 0, 3, addr, None, addr), (pol(), 0, 3, addr, addr, None), (pol(), 0, 3, addr, addr, addr + 16),
           (pol(), 0, 3, addr, addr, addr)]  # the last: everything fine but the NULL handle
    for p, bl, steps, obs, grad, ws in bad:
        rc = fn(None, None if p is None else C.byref(p), bl, steps, obs, grad, ws, 1 << 30, None)
        assert rc == _ffi.ERR_ARG if hasattr(_ffi, "ERR_ARG") else rc != 0, lib.w2a_last_error()
        assert b"w2a_policy_gradient_mlp" in lib.w2a_last_error()
