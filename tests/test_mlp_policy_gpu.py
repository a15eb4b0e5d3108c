"""rollout(kind="mlp") on the GPU (k_rollout_mlp): against the vector oracle's `a = mlp(obs); step(a)` loop in fp64,
against the env's own step() loop, against rollout(kind="linear") as a special case, bit-identical across visiting
orders and group layouts, its refusals, and at full size.
Uniform tables only; the same kernel on ragged episode lengths and slot-27 coefficient rows:
tests/test_table_edges_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import heatalert_oracle as O
from weather2alert_amd import _ffi, policy, synth, tables

pytestmark = pytest.mark.gpu

RETURN_RTOL, RETURN_ATOL = 2e-6, 2e-5  # as tests/test_env_gpu.py
INT_STATE = ("t", "used", "streak", "last_actual", "at_budget")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=6, seed=17, extra_confounder_fips=3)


@pytest.fixture(scope="module")
def ct(sd):
    return tables.compile_from_synth(sd)


def _scale(ct):
    """Per observation column: 1 / spread of the column on synthetic rows (so random networks see O(1) inputs)."""
    s = np.ones(ct.n_obs)
    s[ct.feature_names.index("remaining_budget")] = 0.1
    return s


def _net(ct, hidden, n_out, G, seed):
    rng = np.random.default_rng(seed)
    dims = [ct.n_obs] + list(hidden) + [n_out]
    layers = []
    for i in range(len(dims) - 1):
        W = rng.standard_normal((G, dims[i + 1], dims[i])) * (1.5 / np.sqrt(dims[i]))
        if i == 0:
            W *= _scale(ct)[None, None, :]
        b = rng.standard_normal((G, dims[i + 1])) * 0.5
        layers.append((W.astype(np.float32), b.astype(np.float32)))
    return layers


def _mlp64(layers, activation, obs, g):
    """fp64 logits of the f32 parameters on the f32 observation rows, and each one's near-tie scale
    |b_out| + sum_h |w_out,h h_h| (two outputs folded into row1 - row0 in fp64, as the host does)."""
    act = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0.0))
    h = obs.astype(np.float64)
    for W, b in layers[:-1]:
        W64, b64 = W.astype(np.float64), b.astype(np.float64)
        h = act(np.einsum("noi,ni->no", W64[g], h) + b64[g]) if W.ndim == 3 else act(h @ W64.T + b64)
    Wo, bo = layers[-1]
    Wo, bo = Wo.astype(np.float64), bo.astype(np.float64)
    if Wo.ndim == 2:
        Wo, bo = Wo[None], bo[None]
        g = np.zeros(len(obs), np.int64)
    if Wo.shape[1] == 2:
        Wo, bo = Wo[:, 1:] - Wo[:, :1], bo[:, 1:] - bo[:, :1]
    # the host rounds the folded row to f32 once
    Wo, bo = Wo.astype(np.float32).astype(np.float64)[:, 0], bo.astype(np.float32).astype(np.float64)[:, 0]
    prod = Wo[g] * h
    return prod.sum(axis=1) + bo[g], np.abs(prod).sum(axis=1) + np.abs(bo[g])


def _oracle_for_env(env, V, idx=None):
    st = {k: v.cpu().numpy() for k, v in env.state().items()}
    if idx is not None:
        st = {k: v[idx] for k, v in st.items()}
    V.reset(st["county_w"], st["year_i"], st["coef_col"], st["sample"], st["budget"])
    V._finished = np.zeros(len(st["t"]), bool)
    return st


def _oracle_mlp(V, layers, activation, g, n_steps, T, uniform=None, acc=None):
    """`a = mlp(V.obs); V.step(a)` with fp64 logits; accumulates into acc (ret, alerts, over, alert/attempt days, tie)."""
    n = len(V.t)
    if acc is None:
        acc = dict(ret=np.zeros(n), alerts=np.zeros(n, np.int64), over=np.zeros(n, np.int64),
                   days=np.zeros((n, T), bool), att=np.zeros((n, T), bool), tie=np.zeros(n, bool))
    for _ in range(n_steps):
        live = ~V._finished
        if not live.any():
            break
        z, mag = _mlp64(layers, activation, V.obs.astype(np.float32), g)
        # near-ties by the contract's form (include/w2a.h) with a tenth of its bound -- still ~100x the f32 network's
        # error -- so that random networks leave fewer than 1 % of envs out
        acc["tie"] |= live & (np.abs(z) <= 1e-5 * mag)
        if uniform is None:
            act = z > 0
        else:
            s = 1.0 / (1.0 + np.exp(-z))
            u = uniform(V.t).astype(np.float64)
            act = u < s
            acc["tie"] |= live & (np.abs(s - u) <= 1e-5)
        act = (act & live).astype(np.int64)
        tday, atb = V.t.copy(), V.used == V.budget
        _, r, done, actual = V.step(act)
        acc["ret"] += np.where(live, r, 0.0)
        acc["alerts"] += np.where(live, actual, 0)
        acc["over"] += np.where(live & (act == 1) & atb, 1, 0)
        rows = np.arange(n)
        acc["days"][rows[live & (actual == 1)], tday[live & (actual == 1)]] = True
        acc["att"][rows[live & (act == 1)], tday[live & (act == 1)]] = True
        V._finished = V._finished | (live & done)
    return acc


def _add(tot, out):
    for k in ("return", "alerts", "attempts_over_budget"):
        tot[k] = out[k].cpu().numpy() + tot.get(k, 0)
    return tot


# (hidden widths, activation, output rows, sample): every padding (1 -> 16, 7/9/29 -> 32, 33 -> 64, 64), both layer
# counts, both activations, both output forms, deterministic and sampled decisions
CASES = [((16,), "tanh", 1, False), ((7, 29), "relu", 2, True), ((33,), "relu", 1, True), ((64, 64), "tanh", 2, False),
         ((1,), "tanh", 2, True), ((29, 9), "tanh", 1, False), ((64,), "relu", 2, False), ((40, 64), "relu", 1, True)]


@pytest.mark.parametrize("hidden,activation,n_out,sample", CASES)
def test_mlp_rollout_matches_oracle_policy_loop(dev, sd, ct, hidden, activation, n_out, sample):
    """40 days of rollout(mlp), 10 step() days with random actions, the rest of the episode by rollout(mlp), G = 5 groups
    by an explicit interleaved map: integers, day bitmaps and the observation buffer exact against the oracle's fp64
    loop (envs with a near-tie excepted, < 1 %), returns to the suite's tolerance."""
    from weather2alert_amd import HeatAlertVecEnv

    V = O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years)
    n, gid0, G, seed = 2000 + 37, 300, 5, 11
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=gid0, similar_climate_counties=True)
    env.reset(seed=5, options={"budget": 8})
    st = _oracle_for_env(env, V)
    layers = _net(ct, hidden, n_out, G, seed=len(hidden) * 10 + hidden[0])
    g = (np.arange(n) * 3 + np.arange(n) // 7) % G  # interleaved: most waves hold all five groups
    pol = dict(kind="mlp", layers=layers, activation=activation, group=g, sample=sample, seed=seed)
    uni = (lambda t: O.devrng_policy_uniform_vec(seed, gid0 + np.arange(n), st["episode_no"], t)) if sample else None
    tot = {}
    out = env.rollout(pol, n_steps=40, alert_mask=True)
    assert env.last_rollout_kernel == "k_rollout_mlp" and env.check_status() == 0
    np.testing.assert_allclose(out["group_mean_return"].cpu().numpy(),
                               [out["return"].cpu().numpy()[g == k].mean() for k in range(G)], rtol=1e-5)
    _add(tot, out)
    acc = _oracle_mlp(V, layers, activation, g, 40, ct.T, uniform=uni)
    rng = np.random.default_rng(9)
    for _ in range(10):
        a = (rng.random(n) < 0.3).astype(np.int32)
        env.step(torch.as_tensor(a, device=dev))
        V.step(a)
    out = env.rollout(pol, alert_mask=True)
    _add(tot, out)
    acc_b = _oracle_mlp(V, layers, activation, g, ct.T, ct.T, uniform=uni)
    assert env.check_status() == 0
    assert out["done"].all() and V._finished.all()
    tie = acc["tie"] | acc_b["tie"]
    assert tie.mean() < 0.01, tie.sum()
    ok = ~tie
    alerts_o = acc["alerts"] + acc_b["alerts"]
    assert alerts_o[ok].sum() > 0.05 * n and (alerts_o[ok] < ct.T).any()  # a policy that decides
    np.testing.assert_array_equal(tot["alerts"][ok], alerts_o[ok])
    np.testing.assert_array_equal(tot["attempts_over_budget"][ok], (acc["over"] + acc_b["over"])[ok])
    np.testing.assert_array_equal(out["alert_days"].cpu().numpy()[ok], acc_b["days"][ok])
    np.testing.assert_array_equal(out["attempt_days"].cpu().numpy()[ok], acc_b["att"][ok])
    np.testing.assert_allclose(tot["return"][ok], (acc["ret"] + acc_b["ret"])[ok], rtol=RETURN_RTOL, atol=RETURN_ATOL)
    s = {k: v.cpu().numpy() for k, v in env.state().items()}
    for k, v in (("t", V.t), ("used", V.used), ("streak", V.streak), ("last_actual", V.last_actual),
                 ("at_budget", V.at_budget.astype(np.int64))):
        np.testing.assert_array_equal(s[k][ok], v[ok], err_msg=k)
    np.testing.assert_array_equal(env._obs.cpu().numpy()[ok], V.obs.astype(np.float32)[ok])
    env.close()


def _torch_mlp64(layers, activation, obs, g):
    act = torch.tanh if activation == "tanh" else torch.relu
    h = obs.double()
    for i, (W, b) in enumerate(layers):
        W, b = W.double()[g], b.double()[g]
        h = torch.einsum("noi,ni->no", W, h) + b
        if i < len(layers) - 1:
            h = act(h)
    return h[:, 1] - h[:, 0] if h.shape[1] == 2 else h[:, 0]


@pytest.mark.parametrize("mode", ["order", "no_order", "lockstep_same_step", "disabled", "next_step"])
def test_mlp_rollout_equals_the_envs_step_loop(dev, ct, mode):
    """Two envs from one seed: rollout(mlp) on one, a torch fp64 `mlp(obs) -> step()` loop on the other. Returns, alerts,
    integer state and the final observation agree (envs whose logit ever came near a tie excepted) -- with and without
    the env's rollout order, in lock-step same_step mode over two episodes, with autoreset "disabled" and "next_step"."""
    from weather2alert_amd import HeatAlertVecEnv

    n, G, act_kind = 4096 + 5, 4, ("tanh" if mode != "disabled" else "relu")
    kw = dict(tables=ct, device=dev)
    if mode in ("order", "no_order"):
        kw.update(lockstep=False, autoreset="disabled", rollout_order=(mode == "order"))
    elif mode == "disabled":
        kw.update(autoreset="disabled")
    elif mode == "next_step":
        kw.update(autoreset="next_step")
    A, B = HeatAlertVecEnv(n, **kw), HeatAlertVecEnv(n, **kw)
    A.reset(seed=8)
    B.reset(seed=8)
    layers = _net(ct, (24, 16), 2, G, seed=4)
    g = np.random.default_rng(2).integers(0, G, n)
    pol = dict(kind="mlp", layers=layers, activation=act_kind, group=g)
    tl = [(torch.as_tensor(W, device=dev), torch.as_tensor(b, device=dev)) for W, b in layers]
    gt = torch.as_tensor(g, device=dev).long()
    tie = torch.zeros(n, dtype=torch.bool, device=dev)
    episodes = 2 if mode in ("lockstep_same_step", "next_step") else 1
    for ep in range(episodes):
        if mode == "next_step" and ep == 1:
            B.step(torch.zeros(n, dtype=torch.int32, device=dev))  # the restart call: actions ignored, reward 0
        ua0 = A.state()["used"]
        oa = A.rollout(pol, n_steps=50)
        ob = A.rollout(pol)
        ret_b = torch.zeros(n, dtype=torch.float64, device=dev)
        for _ in range(ct.T):
            z = _torch_mlp64(tl, act_kind, B._obs, gt)
            tie |= z.abs() < 1e-5
            _, r, _, _, _ = B.step((z > 0).to(torch.int32))
            ret_b += r.double()
        assert A.last_rollout_kernel == "k_rollout_mlp"
        ok = ~tie
        assert tie.float().mean() < 0.01
        torch.testing.assert_close((oa["return"] + ob["return"])[ok], ret_b.float()[ok], rtol=RETURN_RTOL,
                                   atol=RETURN_ATOL)
        if mode in ("order", "no_order", "disabled"):
            sa, sb = A.state(), B.state()
            for k in INT_STATE + ("hist14", "finished"):
                assert torch.equal(sa[k][ok], sb[k][ok]), k
            assert torch.equal((oa["alerts"] + ob["alerts"])[ok], (sa["used"] - ua0)[ok])
        assert torch.equal(A._obs[ok], B._obs[ok])
        assert A.check_status() == 0 and B.check_status() == 0
    A.close()
    B.close()


@pytest.mark.parametrize("sample", [False, True])
def test_linear_policy_is_a_special_case(dev, ct, sample):
    """A one-hidden-layer ReLU net with units relu(w.x + b), relu(-(w.x + b)) and output h0 - h1 computes the linear
    logit: decisions and returns equal rollout(kind="linear") with the same w, b, seed and sample (near-ties excepted)."""
    from weather2alert_amd import HeatAlertVecEnv

    n, G = 3000 + 11, 3
    rng = np.random.default_rng(7)
    W = (rng.standard_normal((G, ct.n_obs)) * 0.4 * _scale(ct)).astype(np.float32)
    b = (rng.standard_normal(G) * 0.5).astype(np.float32)
    g = rng.integers(0, G, n)
    W1 = np.stack([W, -W], axis=1)                       # [G, 2, n_obs]
    b1 = np.stack([b, -b], axis=1)                       # [G, 2]
    Wo = np.tile(np.array([[1.0, -1.0]], np.float32), (G, 1, 1))
    mlp = dict(kind="mlp", layers=[(W1, b1), (Wo, np.zeros((G, 1), np.float32))], activation="relu", group=g,
               sample=sample, seed=3)
    lin = dict(kind="linear", weight=W, bias=b, group=g, sample=sample, seed=3)
    A = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", similar_climate_counties=True)
    B = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", similar_climate_counties=True)
    A.reset(seed=2, options={"budget": 6})
    B.reset(seed=2, options={"budget": 6})
    oa = A.rollout(mlp, alert_mask=True)
    ob = B.rollout(lin, alert_mask=True)
    assert A.last_rollout_kernel == "k_rollout_mlp" and B.last_rollout_kernel == "k_rollout_linear"
    # an env whose decisions differ anywhere met a near-tie (f32 network against the fp64 linear chain): < 1 %
    same = ~(oa["attempt_days"] != ob["attempt_days"]).any(dim=1)
    assert float(same.float().mean()) > 0.99
    for k in ("alerts", "attempts_over_budget", "alert_days", "attempt_days", "done"):
        assert torch.equal(oa[k][same], ob[k][same]), k
    torch.testing.assert_close(oa["return"][same], ob["return"][same], rtol=3e-6, atol=3e-5)
    assert bool((oa["alerts"] > 0).any())
    for e in (A, B):
        assert e.check_status() == 0
        e.close()


def _direct(env, P, width, nl, group, order, n_groups, steps, activation=0, sample=0, seed=0):
    """w2a_rollout_mlp called through the C ABI; returns (return, alerts)."""
    n, dev = env.num_envs, env.device
    ret = torch.empty(n, dtype=torch.float32, device=dev)
    alerts = torch.empty(n, dtype=torch.int32, device=dev)
    over = torch.empty(n, dtype=torch.int32, device=dev)
    mp = _ffi.MlpPolicy()
    mp.params, mp.group = P.data_ptr(), group.data_ptr()
    mp.order = None if order is None else order.data_ptr()
    mp.n_groups, mp.n_layers, mp.width, mp.activation = n_groups, nl, width, activation
    mp.sample, mp.require_budget, mp.seed = sample, 0, seed
    _ffi.check(env._lib.w2a_rollout_mlp(env._h, C.byref(mp), steps, env._obs.data_ptr(), ret.data_ptr(),
                                        alerts.data_ptr(), over.data_ptr(), None, None, 0, None, None, env._stream()),
               "w2a_rollout_mlp")
    torch.cuda.synchronize()
    return ret, alerts


def test_outputs_are_bit_identical_across_visiting_orders(dev, ct):
    """One env -> group map; the group-major order (default), the identity order (every wave holds many groups) and a
    shuffled caller order give bit-identical outputs and observation buffers -- through the Python API and through
    w2a_rollout_mlp directly."""
    from weather2alert_amd import HeatAlertVecEnv

    n, G = 5000 + 3, 7
    g = np.random.default_rng(4).integers(0, G, n)
    perm = np.random.default_rng(5).permutation(n)
    for hidden, act in (((64, 64), "tanh"), ((20,), "relu")):
        layers = _net(ct, hidden, 2, G, seed=8)
        res = []
        for order in (None, np.arange(n), perm):
            env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled")
            env.reset(seed=6)
            pol = dict(kind="mlp", layers=layers, activation=act, group=g, sample=True, seed=2)
            if order is not None:
                pol["order"] = order
            o1 = env.rollout(pol, n_steps=33, alert_mask=True)
            o2 = env.rollout(pol, alert_mask=True)
            res.append([o1["return"], o1["alerts"], o2["return"], o2["alerts"], o2["alert_days"], env._obs.clone(),
                        env.state()["used"]])
            assert env.check_status() == 0
            env.close()
        assert int(res[0][1].sum() + res[0][3].sum()) > 0
        for other in res[1:]:
            for a, b in zip(res[0], other):
                assert torch.equal(a, b)
    # the C entry point: order NULL (identity here) against a shuffled order, on two envs from one seed
    a = policy.check_mlp_policy(dict(kind="mlp", layers=_net(ct, (33,), 1, G, seed=9), activation="tanh", group=g),
                                ct.n_obs, n, ct.obs_slot, dev)
    outs = []
    for order in (None, torch.as_tensor(perm, dtype=torch.int32, device=dev), a.order):
        env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", lockstep=False, rollout_order=False)
        env.reset(seed=6)
        r1, a1 = _direct(env, a.params, a.width, a.n_layers, a.group, order, G, 70)
        r2, a2 = _direct(env, a.params, a.width, a.n_layers, a.group, order, G, 200)
        outs.append((r1, a1, r2, a2, env._obs.clone()))
        assert env.check_status() == 0
        env.close()
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert torch.equal(x, y)


def test_mlp_rollout_refusals(dev, ct):
    from weather2alert_amd import HeatAlertVecEnv

    n, G = 512, 2
    layers = _net(ct, (16,), 2, G, seed=5)
    g = np.arange(n) % G
    pol = dict(kind="mlp", layers=layers, activation="tanh", group=g)
    pm = HeatAlertVecEnv(n, tables=ct, device=dev, reward_mode="posterior_mean", autoreset="disabled")
    pm.reset(seed=1)
    with pytest.raises(ValueError, match="sampled"):
        pm.rollout(pol)
    pm.close()
    fx = HeatAlertVecEnv(n, tables=ct, device=dev, fixes=("lag",))
    fx.reset(seed=1)
    with pytest.raises(ValueError, match="faithful"):
        fx.rollout(pol)
    fx.close()
    ok = HeatAlertVecEnv(n, tables=ct, device=dev, fixes=("budget",), autoreset="disabled")
    ok.reset(seed=1)
    ok.rollout(pol, n_steps=3)
    assert ok.check_status() == 0 and ok.last_rollout_kernel == "k_rollout_mlp"
    W1, b1 = layers[0]
    bads = (dict(layers=[(W1[:, :, :-1], b1), layers[1]]), dict(layers=layers * 2), dict(group=g[:-1]),
            dict(group=g + 1), dict(activation="gelu"), dict(layers=[(np.where(W1 > 0, np.inf, W1), b1), layers[1]]),
            dict(layers=[(np.zeros((G, 65, ct.n_obs), np.float32), np.zeros((G, 65), np.float32)),
                         (np.zeros((G, 1, 65), np.float32), np.zeros((G, 1), np.float32))]),
            dict(layers=[layers[0], (np.zeros((G, 3, 16), np.float32), np.zeros((G, 3), np.float32))]),
            dict(order=np.zeros(n, np.int64)))
    for bad in bads:
        with pytest.raises(ValueError):
            ok.rollout({**pol, **bad})
        assert ok.check_status() == 0
    ok.rollout(pol, n_steps=3)
    assert ok.check_status() == 0
    # the C entry point refuses a bad width on a live handle, and the handle stays usable
    mp = _ffi.MlpPolicy()
    P = torch.zeros(policy.mlp_stride(64, 2) * G, dtype=torch.float32, device=dev)
    mp.params, mp.n_groups, mp.n_layers, mp.width, mp.activation = P.data_ptr(), G, 1, 48, 0
    assert ok._lib.w2a_rollout_mlp(ok._h, C.byref(mp), 3, ok._obs.data_ptr(), None, None, None, None, None, 0, None, None,
                                   ok._stream()) == -1
    mp.width, mp.params = 16, P.data_ptr() + 4
    assert ok._lib.w2a_rollout_mlp(ok._h, C.byref(mp), 3, ok._obs.data_ptr(), None, None, None, None, None, 0, None, None,
                                   ok._stream()) == -1
    assert b"aligned" in ok._lib.w2a_last_error()
    ok.rollout(pol, n_steps=2)
    assert ok.check_status() == 0
    # a built-in rollout stopped mid-episode writes no observation rows: the buffer is stale until step() / reset()
    ok.rollout(dict(kind="always"), n_steps=5)
    with pytest.raises(RuntimeError, match="observation buffer"):
        ok.rollout(pol)
    ok.step(torch.zeros(n, dtype=torch.int32, device=dev))
    ok.rollout(pol, n_steps=2)
    ok.load_state_dict(ok.state_dict())
    with pytest.raises(RuntimeError, match="observation buffer"):
        ok.rollout(pol)
    ok.reset(seed=2)
    ok.rollout(pol, n_steps=2)
    assert ok.check_status() == 0
    ok.close()
    no = HeatAlertVecEnv(n, tables=ct, device=dev, write_obs=False)
    no.reset(seed=1)
    with pytest.raises(RuntimeError, match="observation buffer"):
        no.rollout(pol)
    no.close()


def test_mlp_rollout_full_size(dev, sd, ct):
    """1 048 576 envs, G = 1024 random groups, [64, 64] tanh: a strided sample of 4097 envs (the last included) against
    the oracle's fp64 loop; then an SB3-shaped actor through policy.mlp_from_module on the same batch."""
    from weather2alert_amd import HeatAlertVecEnv

    n, G = 1 << 20, 1024
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", similar_climate_counties=True)
    env.reset(seed=77)
    idx = np.unique(np.concatenate([np.arange(0, n, 256), [n - 1]]))
    assert len(idx) == 4097
    V = O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years)
    _oracle_for_env(env, V, idx)
    layers = _net(ct, (64, 64), 2, G, seed=6)
    g = np.random.default_rng(3).integers(0, G, n)
    pol = dict(kind="mlp", layers=layers, activation="tanh", group=torch.as_tensor(g, device=dev))
    o1 = env.rollout(pol, n_steps=100)
    o2 = env.rollout(pol)
    assert env.check_status() == 0 and o2["done"].all()
    acc = _oracle_mlp(V, layers, "tanh", g[idx], ct.T, ct.T)
    ok = ~acc["tie"]
    assert acc["tie"].mean() < 0.01 and ok[-1]
    np.testing.assert_array_equal((o1["alerts"] + o2["alerts"]).cpu().numpy()[idx][ok], acc["alerts"][ok])
    np.testing.assert_allclose((o1["return"] + o2["return"]).cpu().numpy()[idx][ok], acc["ret"][ok], rtol=RETURN_RTOL,
                               atol=RETURN_ATOL)
    s = {k: v.cpu().numpy()[idx] for k, v in env.state().items()}
    for k, v in (("t", V.t), ("used", V.used), ("streak", V.streak), ("last_actual", V.last_actual)):
        np.testing.assert_array_equal(s[k][ok], v[ok], err_msg=k)
    np.testing.assert_array_equal(env._obs.cpu().numpy()[idx][ok], V.obs.astype(np.float32)[ok])
    gm = o2["group_mean_return"].cpu().numpy()
    ret2 = o2["return"].cpu().numpy()
    np.testing.assert_allclose(gm[:3], [ret2[g == k].mean() for k in range(3)], rtol=1e-5)
    # an SB3 PPO actor: policy_net (Linear, Tanh) x 2, then action_net (2 action logits)
    nn = torch.nn
    torch.manual_seed(0)
    actor = nn.Sequential(nn.Linear(ct.n_obs, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 2))
    with torch.no_grad():
        actor[0].weight.mul_(torch.as_tensor(_scale(ct), dtype=torch.float32)[None, :] * 3.0)
    env.reset(seed=78)
    V2 = O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years)
    _oracle_for_env(env, V2, idx)
    out = env.rollout(policy.mlp_from_module(actor))
    assert env.check_status() == 0 and out["done"].all()
    lay = [(m.weight.detach().numpy(), m.bias.detach().numpy()) for m in actor if isinstance(m, nn.Linear)]
    acc = _oracle_mlp(V2, lay, "tanh", np.zeros(len(idx), np.int64), ct.T, ct.T)
    ok = ~acc["tie"]
    assert acc["tie"].mean() < 0.01
    np.testing.assert_array_equal(out["alerts"].cpu().numpy()[idx][ok], acc["alerts"][ok])
    np.testing.assert_allclose(out["return"].cpu().numpy()[idx][ok], acc["ret"][ok], rtol=RETURN_RTOL, atol=RETURN_ATOL)
    env.close()
