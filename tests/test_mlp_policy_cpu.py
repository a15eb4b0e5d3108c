"""CPU checks of rollout(kind="mlp"): the C ABI of w2a_rollout_mlp (struct layout, host-side refusals without a GPU)
and weather2alert_amd/policy.py (argument checks, the packed parameter layout, mlp_from_module, the group order)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from weather2alert_amd import _ffi, build, policy, synth, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


@pytest.fixture(scope="module")
def ct():
    return tables.compile_from_synth(synth.make_synth("linear", n_fips=8, years=[2006, 2007], n_samples=3, seed=2))


def mlp_fp64(params, width, n_layers, activation, xslot, group=None):
    """fp64 logits of the packed buffer, read by the layout documented in include/w2a.h (w2a_mlp_policy)."""
    P = np.asarray(params, np.float64).reshape(-1, policy.mlp_stride(width, n_layers))
    g = np.zeros(len(xslot), np.int64) if group is None else np.asarray(group)
    act = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0.0))
    o = 0
    W1 = P[:, o:o + 32 * width].reshape(-1, 32, width); o += 32 * width
    b1 = P[:, o:o + width]; o += width
    h = act(np.einsum("nk,nku->nu", xslot, W1[g]) + b1[g])
    if n_layers == 2:
        W2 = P[:, o:o + width * width].reshape(-1, width, width); o += width * width
        b2 = P[:, o:o + width]; o += width
        h = act(np.einsum("nk,nku->nu", h, W2[g]) + b2[g])
    wo = P[:, o:o + width]; o += width
    assert (P[:, o + 1:o + 4] == 0).all() and o + 4 == P.shape[1]
    return (h * wo[g]).sum(axis=1) + P[g, o]


def test_mlp_policy_struct_matches_header():
    text = open(os.path.join(ROOT, "include", "w2a.h")).read()
    body = re.search(r"typedef struct w2a_mlp_policy \{(.*?)\} w2a_mlp_policy;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+);", body)
    assert fields == [f for f, _ in _ffi.MlpPolicy._fields_]
    # 3 pointers, 6 int32, 1 uint64
    assert C.sizeof(_ffi.MlpPolicy) == 3 * 8 + 6 * 4 + 8
    assert _ffi.MlpPolicy.n_groups.offset == 24 and _ffi.MlpPolicy.seed.offset == 48
    assert "w2a_rollout_mlp" in _ffi.SYMBOLS
    assert _ffi.ROLLOUT_KERNELS[4] == "k_rollout_mlp"
    assert re.search(r"4 after\s+\*?\s*w2a_rollout_mlp: k_rollout_mlp", text)
    assert re.search(r"W2A_MLP_TANH = 0, W2A_MLP_RELU = 1", text) and _ffi.MLP_ACTIVATIONS == {"tanh": 0, "relu": 1}
    assert "#define W2A_MLP_STRIDE(width, n_layers)" in text
    assert policy.mlp_stride(64, 2) == 32 * 64 + 64 + 64 * 64 + 64 + 64 + 4 == 6340
    assert policy.mlp_stride(16, 1) == 32 * 16 + 16 + 16 + 4 == 548
    assert all(policy.mlp_stride(w, nl) % 4 == 0 for w in (16, 32, 64) for nl in (1, 2))  # 16-B aligned group blocks


def test_rollout_mlp_refuses_bad_arguments_without_gpu(lib):
    buf = (C.c_float * (policy.mlp_stride(64, 2) + 4))()
    base = C.addressof(buf)
    aligned = (base + 15) // 16 * 16
    obs = (C.c_float * 29)()

    def call(p, n_steps=10, ob=obs):
        return lib.w2a_rollout_mlp(None, None if p is None else C.byref(p), n_steps,
                                   C.cast(ob, C.c_void_p) if ob is not None else None,
                                   None, None, None, None, None, 0, None, None, None)

    def pol(**kw):
        p = _ffi.MlpPolicy()
        p.params, p.group, p.order, p.n_groups, p.n_layers, p.width, p.activation = aligned, None, None, 1, 1, 16, 0
        p.sample, p.require_budget, p.seed = 0, 0, 0
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    cases = ((None, 10, obs, b"NULL policy"), (pol(), 0, obs, b"n_steps"), (pol(), -3, obs, b"n_steps"),
             (pol(params=None), 10, obs, b"NULL params"), (pol(n_groups=0), 10, obs, b"n_groups"),
             (pol(width=8), 10, obs, b"width"), (pol(width=48), 10, obs, b"width"), (pol(width=128), 10, obs, b"width"),
             (pol(n_layers=0), 10, obs, b"n_layers"), (pol(n_layers=3), 10, obs, b"n_layers"),
             (pol(activation=2), 10, obs, b"activation"), (pol(activation=-1), 10, obs, b"activation"),
             (pol(sample=2), 10, obs, b"sample"), (pol(require_budget=-1), 10, obs, b"require_budget"),
             (pol(params=aligned + 4), 10, obs, b"16-B aligned"), (pol(), 10, None, b"NULL obs"),
             (pol(), 10, obs, b"NULL handle"))
    for p, n, ob, msg in cases:
        assert call(p, n, ob) == -1
        assert msg in lib.w2a_last_error(), (msg, lib.w2a_last_error())
    for w in (16, 32, 64):  # every valid combination gets as far as the handle
        for nl in (1, 2):
            for a in (0, 1):
                assert call(pol(width=w, n_layers=nl, activation=a, sample=1)) == -1
                assert b"NULL handle" in lib.w2a_last_error()


def _net(rng, n_in, hidden, n_out, G=None, scale=0.7):
    dims = [n_in] + list(hidden) + [n_out]
    lead = () if G is None else (G,)
    return [(rng.standard_normal(lead + (dims[i + 1], dims[i])).astype(np.float32) * scale / np.sqrt(dims[i]),
             rng.standard_normal(lead + (dims[i + 1],)).astype(np.float32) * 0.3) for i in range(len(dims) - 1)]


def _torch_logit(layers, activation, obs, g=None):
    """fp64 torch evaluation of the layers in observation order (Linear convention); two outputs -> row1 - row0."""
    act = torch.tanh if activation == "tanh" else torch.relu
    h = torch.as_tensor(obs, dtype=torch.float64)
    for i, (W, b) in enumerate(layers):
        W, b = torch.as_tensor(W, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
        if W.dim() == 3:
            W, b = W[g], b[g]
            h = torch.einsum("noi,ni->no", W, h) + b
        else:
            h = h @ W.T + b
        if i < len(layers) - 1:
            h = act(h)
    return (h[:, 1] - h[:, 0] if h.shape[1] == 2 else h[:, 0]).numpy()


@pytest.mark.parametrize("hidden", [(1,), (7,), (16,), (29,), (33,), (64,), (7, 29), (16, 33), (64, 64), (1, 64)])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("n_out", [1, 2])
def test_packed_layout_evaluates_to_the_module(ct, hidden, activation, n_out):
    """The packed buffer, evaluated in fp64 by the documented layout on the 32-slot rows, equals the network evaluated in
    observation order: W1 rows in slot order, zero padding to the kernel's width, the folded two-row output."""
    rng = np.random.default_rng(len(hidden) * 100 + hidden[-1] + n_out)
    n_obs, G, n = ct.n_obs, 3, 200
    layers = _net(rng, n_obs, hidden, n_out, G=G)
    P, width, nl, g_n = policy.pack_mlp(layers, ct.obs_slot, n_obs)
    assert (width, nl, g_n) == (policy.mlp_width(hidden), len(hidden), G) and width in (16, 32, 64)
    assert P.dtype == torch.float32 and P.shape == (G, policy.mlp_stride(width, nl))
    obs = rng.standard_normal((n, n_obs)).astype(np.float32)
    s = policy.slot_map(ct.obs_slot, n_obs)
    xslot = np.zeros((n, 32))
    xslot[:, s] = obs
    g = rng.integers(0, G, n)
    got = mlp_fp64(P.numpy(), width, nl, activation, xslot, g)
    ref = _torch_logit(layers, activation, obs, torch.as_tensor(g))
    # the parameters were rounded to f32 once (the folded output row in fp64 first)
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-6)
    # the rows of slots that are no observation column are zero, for any content of those slots
    others = np.setdiff1d(np.arange(32), s)
    W1 = P.numpy()[:, :32 * width].reshape(G, 32, width)
    assert (W1[:, others] == 0).all() and (W1[:, :, hidden[0]:] == 0).all()


def test_shared_and_per_group_layers_broadcast(ct):
    rng = np.random.default_rng(5)
    n_obs = ct.n_obs
    shared = _net(rng, n_obs, (8,), 1)
    per = [(np.stack([shared[0][0]] * 4), np.stack([shared[0][1]] * 4)), shared[1]]
    P1, *_ = policy.pack_mlp(shared, ct.obs_slot, n_obs)
    P4, _, _, G = policy.pack_mlp(per, ct.obs_slot, n_obs)
    assert P1.shape[0] == 1 and G == 4 and torch.equal(P4, P1.expand(4, -1))


def _ok(n_obs, n, G=3, **kw):
    rng = np.random.default_rng(0)
    return dict(kind="mlp", layers=_net(rng, n_obs, (16,), 2, G=G), activation="tanh", group=np.arange(n) % G, **kw)


def test_mlp_policy_argument_checks(ct):
    n_obs, n = ct.n_obs, 10
    a = policy.check_mlp_policy(_ok(n_obs, n), n_obs, n, ct.obs_slot, "cpu")
    assert a.n_groups == 3 and a.width == 16 and a.n_layers == 1 and a.activation == "tanh"
    assert a.params.shape == (3, policy.mlp_stride(16, 1)) and a.group.dtype == torch.int32
    assert a.order.dtype == torch.int32 and torch.equal(a.order, policy.group_order(a.group))
    assert a.sample is False and a.require_budget is False and a.seed == 0
    rng = np.random.default_rng(1)
    one = policy.check_mlp_policy(dict(kind="mlp", layers=_net(rng, n_obs, (64, 64), 1), activation="relu"), n_obs, n,
                                  ct.obs_slot, "cpu")
    assert one.group is None and one.order is None and one.n_layers == 2 and one.width == 64
    perm = np.random.default_rng(2).permutation(n)
    assert torch.equal(policy.check_mlp_policy(_ok(n_obs, n, order=perm), n_obs, n, ct.obs_slot, "cpu").order,
                       torch.as_tensor(perm, dtype=torch.int32))
    L = _ok(n_obs, n)["layers"]
    bad = [
        dict(layers=_net(rng, n_obs, (16, 16, 16), 1, G=3)),                 # 3 hidden layers
        dict(layers=_net(rng, n_obs, (65,), 1, G=3)),                        # too wide
        dict(layers=_net(rng, n_obs, (16, 65), 1, G=3)),                     # too wide
        dict(layers=_net(rng, n_obs, (16,), 3, G=3)),                        # 3 output rows
        dict(layers=[L[1]]),                                                 # no hidden layer
        dict(layers=_net(rng, n_obs + 1, (16,), 1, G=3)),                    # wrong input width
        dict(layers=[L[0], (L[1][0][:, :, :-1], L[1][1])]),                  # layers do not chain
        dict(layers=[(L[0][0], L[0][1][:, :-1]), L[1]]),                     # bias does not match
        dict(layers=[L[0], (L[1][0][:2], L[1][1][:2])]),                     # layers disagree on G
        dict(layers=[(np.where(L[0][0] > 0, np.nan, L[0][0]), L[0][1]), L[1]]),  # non-finite
        dict(layers=[L[0], (L[1][0], np.full((3, 2), np.inf, np.float32))]),     # non-finite
        dict(layers=[(L[0][0].astype(np.float64) * 1e300, L[0][1]), L[1]]),  # not finite as float32
        dict(layers=[L[0], (np.ones((3, 2, 16)) * np.array([-3e38, 3e38])[None, :, None], L[1][1])]),  # fold overflows
        dict(layers="nope"),
        dict(layers=[L[0], (L[1][0],)]),                                     # not a pair
        dict(activation="sigmoid"),                                          # unknown activation
        dict(group=np.arange(n + 1) % 3),                                    # group not [num_envs]
        dict(group=np.full(n, 3)),                                           # out of range
        dict(group=np.full(n, -1)),                                          # out of range
        dict(group=np.zeros(n, np.float32)),                                 # not integer
        dict(group=None),                                                    # G > 1 needs groups
        dict(order=np.zeros(n, np.int64)),                                   # not a permutation
        dict(order=np.arange(n - 1)),                                        # wrong length
        dict(sample=1),                                                      # not a bool
        dict(seed=1.5),                                                      # not an int
        dict(weight=1),                                                      # unknown key
        dict(layers=None),                                                   # missing
    ]
    for kw in bad:
        p = {**_ok(n_obs, n), **kw}
        if "group" in kw and kw["group"] is None:
            del p["group"]
        if "layers" in kw and kw["layers"] is None:
            del p["layers"]
        with pytest.raises(ValueError):
            policy.check_mlp_policy(p, n_obs, n, ct.obs_slot, "cpu")


def test_mlp_from_module(ct):
    n_obs = ct.n_obs
    torch.manual_seed(0)
    nn = torch.nn
    # an SB3 PPO actor: policy_net (Linear, Tanh, Linear, Tanh) then action_net (Linear -> 2 action logits)
    policy_net = nn.Sequential(nn.Linear(n_obs, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh())
    actor = nn.Sequential(*policy_net, nn.Linear(64, 2))
    pol = policy.mlp_from_module(actor)
    assert pol["kind"] == "mlp" and pol["activation"] == "tanh" and len(pol["layers"]) == 3 and "group" not in pol
    a = policy.check_mlp_policy(pol, n_obs, 5, ct.obs_slot, "cpu")
    obs = torch.randn(50, n_obs)
    s = policy.slot_map(ct.obs_slot, n_obs)
    xslot = np.zeros((50, 32))
    xslot[:, s] = obs.numpy()
    with torch.no_grad():
        q = actor.double()(obs.double())
    np.testing.assert_allclose(mlp_fp64(a.params.numpy(), a.width, a.n_layers, "tanh", xslot), (q[:, 1] - q[:, 0]).numpy(),
                               rtol=1e-5, atol=1e-5)
    # nested Sequential, ReLU, one output, no bias, with a group map
    m = nn.Sequential(nn.Sequential(nn.Linear(n_obs, 7), nn.ReLU()), nn.Linear(7, 1, bias=False))
    p2 = policy.mlp_from_module(m, group=np.zeros(5, np.int64))
    assert p2["activation"] == "relu" and p2["group"] is not None and (p2["layers"][1][1] == 0).all()
    assert policy.check_mlp_policy(p2, n_obs, 5, ct.obs_slot, "cpu").width == 16
    # the module's parameters are copied: later training does not change the policy
    with torch.no_grad():
        m[1].weight.add_(1.0)
    assert not torch.equal(p2["layers"][1][0], m[1].weight)
    for bad in (nn.Linear(n_obs, 1),                                                     # not a Sequential
                nn.Sequential(nn.Linear(n_obs, 8), nn.Sigmoid(), nn.Linear(8, 1)),      # unsupported activation
                nn.Sequential(nn.Linear(n_obs, 8), nn.Tanh(), nn.Linear(8, 8), nn.ReLU(), nn.Linear(8, 1)),  # mixed
                nn.Sequential(nn.Linear(n_obs, 8), nn.Linear(8, 1)),                     # no activation
                nn.Sequential(nn.Linear(n_obs, 8), nn.Tanh(), nn.Linear(8, 1), nn.Tanh()),  # trailing activation
                nn.Sequential(*[x for _ in range(3) for x in (nn.Linear(n_obs if _ == 0 else 8, 8), nn.Tanh())],
                              nn.Linear(8, 1)),                                          # three hidden layers
                nn.Sequential(nn.Linear(n_obs, 8), nn.Tanh(), nn.Linear(8, 3)),          # three outputs
                nn.Sequential(nn.Linear(n_obs, 8), nn.Tanh(), nn.Dropout(), nn.Linear(8, 1))):
        with pytest.raises(ValueError):
            policy.mlp_from_module(bad)


def test_group_order_is_a_stable_group_contiguous_permutation():
    rng = np.random.default_rng(3)
    g = torch.as_tensor(rng.integers(0, 37, 5000), dtype=torch.int32)
    o = policy.group_order(g)
    assert o.dtype == torch.int32 and torch.equal(torch.sort(o).values, torch.arange(5000, dtype=torch.int32))
    go = g[o.long()]
    assert bool((go[1:] >= go[:-1]).all())  # group-contiguous, ascending
    for k in range(37):  # stable: each group's envs in ascending id order
        ids = o[go == k]
        assert bool((ids[1:] > ids[:-1]).all())
