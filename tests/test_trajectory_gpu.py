"""rollout(kind="linear" | "mlp", record=True) on the GPU: the recorded trajectory against the vector oracle's
`a = policy(obs); step(a)` loop and against the env's own step() loop, recording changing nothing else, chaining,
order independence, the MLP against torch, refusals and full size.
Uniform tables only; the same kernel on ragged episode lengths and slot-27 coefficient rows:
tests/test_table_edges_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import heatalert_oracle as O
from weather2alert_amd import policy, synth, tables

pytestmark = pytest.mark.gpu

REWARD_TOL = 1e-5  # the suite's per-step bar
TRAJ_KEYS = ("obs", "action", "logit", "reward", "valid", "terminated", "alert")


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


def _params(ct, G, seed, scale=0.4):
    """Random linear parameters with a sensible alert rate (as tests/test_linear_policy_gpu.py)."""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((G, ct.n_obs)) * scale).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] *= 0.1
    b = (rng.standard_normal(G) * 0.5).astype(np.float32)
    return W, b


def _net(ct, hidden, n_out, G, seed):
    """Random MLP layers [G, out, in] (as tests/test_mlp_policy_gpu.py)."""
    rng = np.random.default_rng(seed)
    dims = [ct.n_obs] + list(hidden) + [n_out]
    layers = []
    for i in range(len(dims) - 1):
        W = rng.standard_normal((G, dims[i + 1], dims[i])) * (1.5 / np.sqrt(dims[i]))
        if i == 0:
            W[:, :, ct.feature_names.index("remaining_budget")] *= 0.1
        b = rng.standard_normal((G, dims[i + 1])) * 0.5
        layers.append((W.astype(np.float32), b.astype(np.float32)))
    return layers


def _mlp64(layers, activation, obs, g):
    """fp64 logits of the f32 parameters on f32 rows and each one's near-tie scale |b_out| + sum_h |w_out,h h_h| (two
    outputs folded into row1 - row0 and rounded to f32 once, as the host does)."""
    act = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0.0))
    h = obs.astype(np.float64)
    for W, b in layers[:-1]:
        h = act(np.einsum("noi,ni->no", W.astype(np.float64)[g], h) + b.astype(np.float64)[g])
    Wo, bo = layers[-1]
    Wo, bo = Wo.astype(np.float64), bo.astype(np.float64)
    if Wo.shape[1] == 2:
        Wo, bo = Wo[:, 1:] - Wo[:, :1], bo[:, 1:] - bo[:, :1]
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


def _oracle_record(V, logit_fn, S, tie_rel, uniform=None, require_budget=False):
    """`a = policy(V.obs); V.step(a)` for S days, recorded like rollout(record=True): numpy arrays [S(+1), n, ...], the
    fp64 logits, the uniforms (sample) and a per-env near-tie flag (an env with a tie anywhere is left out: after a
    differing decision its trajectory legitimately diverges)."""
    n, n_obs = V.obs.shape
    R = dict(obs=np.zeros((S + 1, n, n_obs), np.float32), action=np.zeros((S, n), np.uint8), logit=np.zeros((S, n)),
             mag=np.zeros((S, n)), reward=np.zeros((S, n)), valid=np.zeros((S, n), bool),
             terminated=np.zeros((S, n), bool), alert=np.zeros((S, n), bool), u=np.zeros((S, n)),
             tie=np.zeros(n, bool), t0=V.t.copy())
    for s in range(S):
        live = ~V._finished
        R["obs"][s] = V.obs.astype(np.float32)
        if not live.any():
            continue
        z, mag = logit_fn(R["obs"][s])
        if uniform is None:
            act = z > 0
            R["tie"] |= live & (np.abs(z) <= tie_rel * mag)
        else:
            sg = 1.0 / (1.0 + np.exp(-z))
            u = uniform(V.t).astype(np.float64)
            act = u < sg
            R["tie"] |= live & (np.abs(sg - u) <= 1e-5)
            R["u"][s] = u
        if require_budget:
            act &= (V.budget - V.used) > 0
        act = (act & live).astype(np.int64)
        _, r, done, actual = V.step(act)
        R["action"][s] = np.where(live, act, 0)
        R["logit"][s], R["mag"][s], R["reward"][s] = z, mag, r
        R["valid"][s], R["terminated"][s], R["alert"][s] = live, live & done, live & (actual == 1)
        V._finished = V._finished | (live & done)
    R["obs"][S] = V.obs.astype(np.float32)
    return R


def _np(tr):
    return {k: v.cpu().numpy() for k, v in tr.items()}


def _check_against_oracle(tr, R, kind, sample, require_budget):
    ok = ~R["tie"]
    assert R["tie"].mean() < 0.02, R["tie"].sum()
    v = R["valid"][:, ok]
    for k in ("valid", "terminated", "alert", "action"):
        np.testing.assert_array_equal(tr[k][:, ok], R[k][:, ok], err_msg=k)
    assert R["alert"][:, ok].any() and (R["alert"][:, ok] < v).any()  # a policy that decides
    # flags are False wherever the env took no step
    assert not (tr["terminated"] & ~tr["valid"]).any() and not (tr["alert"] & ~tr["valid"]).any()
    np.testing.assert_array_equal(tr["obs"][:-1, ok][v], R["obs"][:-1, ok][v])
    np.testing.assert_allclose(tr["reward"][:, ok][v], R["reward"][:, ok][v], rtol=REWARD_TOL, atol=REWARD_TOL)
    lg, z, mag = tr["logit"][:, ok][v].astype(np.float64), R["logit"][:, ok][v], R["mag"][:, ok][v]
    if kind == "linear":  # the fp64 logit rounded to f32
        assert (np.abs(lg - z) <= 1e-6 * np.abs(z) + 1e-9 * mag).all()
    else:  # the f32 network, within the near-tie band of include/w2a.h
        assert (np.abs(lg - z) <= 1e-5 * mag).all()
    if sample:
        u = R["u"][:, ok][v]
        sg = 1.0 / (1.0 + np.exp(-lg))
        pred = u < sg
        a = tr["action"][:, ok][v].astype(bool)
        if require_budget:
            assert not (a & ~pred).any()  # forced off at most
        else:
            clear = np.abs(sg - u) > 1e-6
            np.testing.assert_array_equal(a[clear], pred[clear])


def _policy(ct, kind, G, g, sample, require_budget, seed=11, hidden=(16,)):
    if kind == "linear":
        W, b = _params(ct, G, 3)
        pol = dict(kind="linear", weight=W, bias=b, group=g, sample=sample, seed=seed, require_budget=require_budget)
        W64, b64 = W.astype(np.float64)[g], b.astype(np.float64)[g]

        def fn(obs):
            prod = obs.astype(np.float64) * W64
            return prod.sum(axis=1) + b64, np.abs(prod).sum(axis=1) + np.abs(b64)
        return pol, fn, 1e-9
    layers = _net(ct, hidden, 2, G, 5)
    pol = dict(kind="mlp", layers=layers, activation="tanh", group=g, sample=sample, seed=seed,
               require_budget=require_budget)
    return pol, (lambda obs: _mlp64(layers, "tanh", obs, g)), 1e-5


@pytest.mark.parametrize("require_budget", [False, True])
@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_trajectory_matches_oracle_policy_loop(dev, sd, ct, kind, sample, require_budget):
    """A whole episode recorded in one call, G = 3 groups: obs bit-equal, actions and flags exact, rewards and logits
    within their bars, against the oracle's `a = policy(obs); step(a)` loop (near-tie envs excepted)."""
    from weather2alert_amd import HeatAlertVecEnv

    V = O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years)
    n, gid0, G, seed = 1500 + 29, 100, 3, 11
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=gid0, similar_climate_counties=True)
    env.reset(seed=5, options={"budget": 6})
    st = _oracle_for_env(env, V)
    g = np.random.default_rng(1).integers(0, G, n)
    pol, fn, tie_rel = _policy(ct, kind, G, g, sample, require_budget, seed)
    uni = (lambda t: O.devrng_policy_uniform_vec(seed, gid0 + np.arange(n), st["episode_no"], t)) if sample else None
    out = env.rollout(pol, record=True)
    assert env.check_status() == 0 and out["done"].all()
    tr = _np(out["trajectory"])
    S = ct.T
    assert tr["obs"].shape == (S + 1, n, ct.n_obs) and tr["obs"].dtype == np.float32
    for k, dt in (("action", np.uint8), ("logit", np.float32), ("reward", np.float32), ("valid", np.bool_),
                  ("terminated", np.bool_), ("alert", np.bool_)):
        assert tr[k].shape == (S, n) and tr[k].dtype == dt, k
    R = _oracle_record(V, fn, S, tie_rel, uniform=uni, require_budget=require_budget)
    _check_against_oracle(tr, R, kind, sample, require_budget)
    np.testing.assert_array_equal(tr["obs"][0], R["obs"][0])  # the buffer on entry
    np.testing.assert_array_equal(tr["obs"][S], env._obs.cpu().numpy())  # the buffer as the call left it
    assert tr["terminated"].sum(axis=0).tolist() == [1] * n  # every env's episode ended exactly once
    env.close()


def _step_loop_record(env, W, b, g, days, dev):
    """The env's own `policy(obs) -> step()` loop with fp64 logits: the obs it held before every step, the rewards."""
    gi = torch.as_tensor(g, device=dev).long()
    W64, b64 = torch.as_tensor(W, dtype=torch.float64, device=dev)[gi], torch.as_tensor(b, dtype=torch.float64, device=dev)[gi]
    obs, rew = [], []
    for _ in range(days):
        obs.append(env._obs.clone())
        z = (env._obs.double() * W64).sum(dim=1) + b64
        _, r, _, _, _ = env.step((z > 0).to(torch.int32))
        rew.append(r.clone())
    return torch.stack(obs), torch.stack(rew)


@pytest.mark.parametrize("mode", ["order", "no_order", "lockstep_same_step", "disabled", "next_step"])
def test_trajectory_equals_the_envs_step_loop(dev, ct, mode):
    """Two envs from one seed: rollout(linear, record=True) on one, a torch `policy(obs) -> step()` loop on the other:
    obs[s] is what step() returned before decision s, rewards within the bar -- in every autoreset mode."""
    from weather2alert_amd import HeatAlertVecEnv

    n, G = 2048 + 5, 4
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
    W, b = _params(ct, G, 4)
    g = np.random.default_rng(2).integers(0, G, n)
    pol = dict(kind="linear", weight=W, bias=b, group=g)
    for ep in range(2 if mode in ("lockstep_same_step", "next_step") else 1):
        if mode == "next_step" and ep == 1:
            B.step(torch.zeros(n, dtype=torch.int32, device=dev))  # the restart call: actions ignored, reward 0
        tr = A.rollout(pol, record=True)["trajectory"]
        obs_b, rew_b = _step_loop_record(B, W, b, g, ct.T, dev)
        v = tr["valid"]
        assert v.any()
        assert torch.equal(tr["obs"][:-1][v], obs_b[v])
        torch.testing.assert_close(tr["reward"][v], rew_b[v], rtol=REWARD_TOL, atol=REWARD_TOL)
        if mode != "lockstep_same_step":  # no reset after the call: obs[S] is the buffer both envs hold
            assert torch.equal(tr["obs"][-1], A._obs) and torch.equal(A._obs, B._obs)
        assert A.check_status() == 0 and B.check_status() == 0
    A.close()
    B.close()


def _mlp_policy(ct, G, g, sample=True):
    return dict(kind="mlp", layers=_net(ct, (16,), 2, G, 7), activation="tanh", group=g, sample=sample, seed=3)


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_recording_changes_nothing(dev, ct, kind):
    """record=True against record=False on identical envs: every output, the state, the obs buffer and final_return
    bit-equal, in two chained calls; the recorded rewards summed day by day in f32 are out["return"] bit for bit."""
    from weather2alert_amd import HeatAlertVecEnv

    n, G = 3000 + 7, 3
    A = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled")
    B = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled")
    A.reset(seed=4, options={"budget": 5})
    B.reset(seed=4, options={"budget": 5})
    g = np.random.default_rng(5).integers(0, G, n)
    if kind == "linear":
        W, b = _params(ct, G, 6)
        pol = dict(kind="linear", weight=W, bias=b, group=g, sample=True, seed=2)
    else:
        pol = _mlp_policy(ct, G, g)
    for steps in (37, None):
        oa = A.rollout(pol, n_steps=steps, alert_mask=True, record=True)
        ob = B.rollout(pol, n_steps=steps, alert_mask=True)
        assert set(oa) - set(ob) == {"trajectory"} and "trajectory" not in ob
        for k, v in ob.items():
            a_ = oa[k]
            if v.is_floating_point():
                a_, v = a_.nan_to_num(7.0), v.nan_to_num(7.0)
            assert torch.equal(a_, v), k
        sa, sb = A.state(), B.state()
        for k in sb:
            assert torch.equal(sa[k], sb[k]), k
        assert torch.equal(A._obs, B._obs) and torch.equal(A._final_return, B._final_return)
        tr = oa["trajectory"]
        ret = torch.zeros(n, dtype=torch.float32, device=dev)
        for s in range(tr["reward"].shape[0]):
            ret = torch.where(tr["valid"][s], ret + tr["reward"][s], ret)
        assert torch.equal(ret, oa["return"])
        assert torch.equal(tr["alert"].sum(0).to(torch.int32), oa["alerts"])
        assert A.check_status() == 0
    A.close()
    B.close()


def _cat(t1, t2):
    return {k: torch.cat([t1[k][:-1], t2[k]]) if k == "obs" else torch.cat([t1[k], t2[k]]) for k in TRAJ_KEYS}


def _assert_traj_equal(a, b):
    v = b["valid"]
    for k in ("valid", "terminated", "alert"):
        assert torch.equal(a[k], b[k]), k
    for k in ("action", "logit", "reward"):
        assert torch.equal(a[k][v], b[k][v]), k
    assert torch.equal(a["obs"][:-1][v], b["obs"][:-1][v])
    assert torch.equal(a["obs"][-1], b["obs"][-1])


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_trajectory_chains(dev, ct, kind):
    """Calls of k and S - k days record what one call of S days does, bit for bit, and obs[S] of the first is obs[0]
    of the second. In lock-step same_step mode a second whole-episode call records the next episode, and obs[S] of
    the first is the pre-reset row (the terminal step leaves the previous row)."""
    from weather2alert_amd import HeatAlertVecEnv

    n, G, S, k = 2500 + 3, 2, ct.T, 41
    g = np.arange(n) % G
    if kind == "linear":
        W, b = _params(ct, G, 8)
        pol = dict(kind="linear", weight=W, bias=b, group=g, sample=True, seed=9)
    else:
        pol = _mlp_policy(ct, G, g)
    A = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled")
    B = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled")
    A.reset(seed=12)
    B.reset(seed=12)
    t1 = A.rollout(pol, n_steps=k, record=True)["trajectory"]
    t2 = A.rollout(pol, n_steps=S - k, record=True)["trajectory"]
    tb = B.rollout(pol, n_steps=S, record=True)["trajectory"]
    assert torch.equal(t1["obs"][k], t2["obs"][0])
    _assert_traj_equal(_cat(t1, t2), tb)
    A.close()
    B.close()
    # lock step, same_step autoreset: two whole episodes
    L = HeatAlertVecEnv(n, tables=ct, device=dev)
    L.reset(seed=13)
    o1 = L.rollout(pol, record=True)
    after = L._obs.clone()  # the first observation of the next episode
    o2 = L.rollout(pol, record=True)
    e1, e2 = o1["trajectory"], o2["trajectory"]
    assert o1["done"].all() and e1["terminated"].any(0).all() and e2["valid"].any()
    assert torch.equal(e2["obs"][0], after)
    last = e1["valid"].sum(0).long() - 1  # every env's terminal call-day
    rows = torch.arange(n, device=dev)
    assert torch.equal(e1["obs"][-1], e1["obs"][last, rows])  # pre-reset: the row the terminal step kept
    assert not torch.equal(e1["obs"][-1], e2["obs"][0])
    assert L.check_status() == 0
    L.close()


def test_trajectory_is_order_independent(dev, ct):
    """Bit-identical trajectories with the visiting order on and off (linear, mlp), and for mlp under two group
    layouts that give every env the same network."""
    from weather2alert_amd import HeatAlertVecEnv

    n, G = 3000 + 1, 4
    g = np.random.default_rng(6).integers(0, G, n)
    W, b = _params(ct, G, 10)
    lin = dict(kind="linear", weight=W, bias=b, group=g, sample=True, seed=4)
    layers = _net(ct, (32, 32), 2, G, 9)
    perm = np.array([2, 0, 3, 1])  # group k's network moves to id perm[k]
    inv = np.argsort(perm)
    mlp1 = dict(kind="mlp", layers=layers, activation="tanh", group=g, sample=True, seed=4)
    mlp2 = dict(mlp1, layers=[(W_[inv], b_[inv]) for W_, b_ in layers], group=perm[g])
    runs = {}
    for name, order, pol in (("lin_on", True, lin), ("lin_off", False, lin), ("mlp_on", True, mlp1),
                             ("mlp_off", False, mlp1), ("mlp_perm", True, mlp2)):
        env = HeatAlertVecEnv(n, tables=ct, device=dev, lockstep=False, autoreset="disabled", rollout_order=order)
        env.reset(seed=21)
        runs[name] = env.rollout(pol, n_steps=90, record=True)["trajectory"]
        assert env.check_status() == 0
        env.close()
    for a, b_ in (("lin_on", "lin_off"), ("mlp_on", "mlp_off"), ("mlp_on", "mlp_perm")):
        _assert_traj_equal(runs[a], runs[b_])


def test_mlp_trajectory_matches_torch_forward(dev, ct):
    """policy.mlp_from_module of an SB3-shaped [64, 64] tanh actor with two outputs: torch's f32 forward on the recorded
    obs reproduces the recorded logit (row1 - row0) within the near-tie band."""
    from weather2alert_amd import HeatAlertVecEnv

    torch.manual_seed(0)
    actor = torch.nn.Sequential(torch.nn.Linear(ct.n_obs, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64),
                                torch.nn.Tanh(), torch.nn.Linear(64, 2)).to(dev)
    n = 2000 + 9
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled")
    env.reset(seed=3)
    out = env.rollout(policy.mlp_from_module(actor) | {"sample": True}, record=True)
    tr = out["trajectory"]
    v = tr["valid"]
    x = tr["obs"][:-1][v]
    with torch.no_grad():
        y = actor(x)
        z32 = y[:, 1] - y[:, 0]
        a64 = actor.double()
        h = a64[:4](x.double())
        wo = a64[4].weight[1] - a64[4].weight[0]
        bo = a64[4].bias[1] - a64[4].bias[0]
        mag = (h * wo).abs().sum(1) + bo.abs()
    assert (tr["logit"][v] - z32).abs().le(1e-5 * mag.float()).all()
    lp = policy.action_log_prob(tr["logit"][v], tr["action"][v])
    ref = torch.distributions.Categorical(logits=y).log_prob(tr["action"][v].long())
    torch.testing.assert_close(lp, ref, rtol=1e-4, atol=1e-4)
    env.close()


def test_record_refusals(dev, ct):
    """record=True with a built-in kind, and the posterior-mean reward: ValueError before anything runs."""
    from weather2alert_amd import HeatAlertVecEnv

    n = 512
    W, b = _params(ct, 1, 5)
    pol = dict(kind="linear", weight=W, bias=b)
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled")
    env.reset(seed=1)
    t0 = env.state()["t"].clone()
    for builtin in (dict(kind="never"), dict(kind="always"), dict(kind="bernoulli", p=0.2),
                    dict(kind="threshold", feature="heat_qi", threshold=0.8)):
        with pytest.raises(ValueError, match="record=True"):
            env.rollout(builtin, n_steps=3, record=True)
    assert torch.equal(env.state()["t"], t0)
    env.rollout(pol, n_steps=2, record=True)  # the env is still usable
    assert env.check_status() == 0
    env.close()
    pm = HeatAlertVecEnv(n, tables=ct, device=dev, reward_mode="posterior_mean", autoreset="disabled")
    pm.reset(seed=1)
    for p in (pol, _mlp_policy(ct, 1, None)):
        with pytest.raises(ValueError, match="sampled"):
            pm.rollout(p, record=True)
    pm.close()


def test_trajectory_full_size(dev, sd, ct):
    """1 048 576 envs, linear sampled, one whole episode: a strided sample of envs against the oracle, and
    valid.sum() == sum(n_days - t0)."""
    from weather2alert_amd import HeatAlertVecEnv

    n, seed = 1 << 20, 5
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", similar_climate_counties=True)
    env.reset(seed=77)
    st = {k: v.cpu().numpy() for k, v in env.state().items()}
    idx = np.unique(np.concatenate([np.arange(0, n, 1021), [n - 1]]))
    V = O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years)
    _oracle_for_env(env, V, idx)
    pol, fn, tie_rel = _policy(ct, "linear", 1, np.zeros(len(idx), np.int64), True, False, seed)
    out = env.rollout({k: v for k, v in pol.items() if k != "group"}, record=True)
    assert env.check_status() == 0 and out["done"].all()
    tr = out["trajectory"]
    assert int(tr["valid"].sum()) == int((st["n_days"].astype(np.int64) - st["t"]).sum())
    sub = {k: v[:, torch.as_tensor(idx, device=dev)].cpu().numpy() for k, v in tr.items()}
    uni = lambda t: O.devrng_policy_uniform_vec(seed, idx, st["episode_no"][idx], t)  # noqa: E731
    R = _oracle_record(V, fn, ct.T, tie_rel, uniform=uni)
    _check_against_oracle(sub, R, "linear", True, False)
    del tr, out
    env.close()
