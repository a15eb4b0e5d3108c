"""imitation_gradient() (k_imitation_linear; k_im_pass1 + the second pass of w2a_policy_gradient_mlp) against the fp64
restatement (tests/imitation_restatement.py). The reference never touches the kernels under test: an identical twin
from the same seed is stepped day by day through step() with the schedule's actions, every env read on its own days
only, and the rows it returns go to the restatement. Every comparison requires |g - g_ref| <= bound for every
component, |ll - ll_ref| <= its bound and equal day counts, and prints the largest ratio to the bound."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from imitation_restatement import imitation_linear_fp64, imitation_mlp_fp64  # noqa: E402
from policy_gradient_mlp_cases import MATRIX, net as case_net  # noqa: E402

from weather2alert_amd import policy, synth, tables  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def data():
    """name -> (compiled tables, env keywords, reset seed, reset options)"""
    sd = synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=6, seed=17, extra_confounder_fips=3)
    out = {"synth": (tables.compile_from_synth(sd), dict(similar_climate_counties=True), 5, {"budget": 10}),
           "mini": (tables.CompiledTables.load_npz(os.path.join(GOLDEN, "mini_compiled.npz")), {}, 5, {"budget": 10})}
    for name, tb in E.make_tables().items():
        out[name] = (tb.ct, dict(similar_climate_counties=True), E.RESET[name]["seed"], dict(E.RESET[name]["opts"]))
    short = synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=6, n_days=12, seed=23, extra_confounder_fips=3)
    out["short"] = (tables.compile_from_synth(short), dict(similar_climate_counties=True), 79, {"budget": 4})
    return out


def _make(dev, data, name, n, **kw):
    from weather2alert_amd import HeatAlertVecEnv

    ct, ekw, seed, opts = data[name]
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=E.GID0, **{**ekw, **kw})
    env.reset(seed=seed, options=dict(opts))
    return env


def _prefix_policy(ct):
    """a sampled linear policy for the days before the call: alerts, so streaks and a non-empty 14-day window"""
    rng = np.random.default_rng(9)
    W = (rng.standard_normal((1, ct.n_obs)) * 0.2).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] *= 0.1
    return dict(kind="linear", weight=W, bias=np.array([0.3], np.float32), sample=True, seed=4)


def _advance(env, ct, days):
    """the days before the call, the same for every twin: a rollout of _prefix_policy, or (reward_mode="posterior_mean",
    which has no linear rollout) step() with fixed random actions"""
    if env.reward_mode == "sampled":
        env.rollout(_prefix_policy(ct), n_steps=days)
        return
    rng = np.random.default_rng(13)
    for _ in range(days):
        env.step(torch.as_tensor((rng.random(env.num_envs) < 0.4).astype(np.int32), device=env.device))


def _schedule(kind, env, n, T):
    if kind == "hindsight":
        return env.hindsight_optimum()["alert_days"]
    if kind == "zeros":
        return torch.zeros((n, T), dtype=torch.bool, device=env.device)
    if kind == "ones":
        return torch.ones((n, T), dtype=torch.bool, device=env.device)
    return torch.as_tensor(np.random.default_rng(21).random((n, T)) < 0.35, device=env.device)


def _weights(n, kind):
    if kind is None:
        return None
    w = np.random.default_rng(8).standard_normal(n).astype(np.float32)  # negative values
    w[::5] = 0.0
    return w


def _step_reference(env, sched, S, require_budget):
    """`env` stepped through step() along `sched` (attempts by day of the episode) for at most S days from where it
    stands; every env is read on its own days only (step() goes on shifting the history of finished envs of a ragged
    batch). Returns numpy obs f64 [S, n, n_obs] (the row held before decision s), labels / valid / forced [S, n]."""
    n, dv = env.num_envs, env.device
    rows = torch.arange(n, device=dv)
    fin = env.state()["finished"].bool()
    R = dict(obs=torch.zeros((S, n, env._obs.shape[1]), dtype=torch.float64, device=dv),
             labels=torch.zeros((S, n), dtype=torch.bool, device=dv), valid=torch.zeros((S, n), dtype=torch.bool, device=dv),
             forced=torch.zeros((S, n), dtype=torch.bool, device=dv))
    for s in range(S):
        if bool(fin.all()):
            break
        st = env.state()
        R["obs"][s] = env._obs.double()
        R["valid"][s] = ~fin
        R["labels"][s] = sched[rows, st["t"].long().clamp(max=sched.shape[1] - 1)] & ~fin
        if require_budget:
            R["forced"][s] = ((st["budget"] - st["used"]) <= 0) & ~fin
        act = (R["labels"][s] & ~R["forced"][s]).to(torch.int32)
        term = env.step(act)[2]
        fin = fin | term.bool()
    return {k: v.cpu().numpy() for k, v in R.items()}, fin


def _ratio(diff, bound):
    return float(np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0)).max())


def _check_ll(out, ref, what):
    ll, days = out["log_likelihood"].double().cpu().numpy(), out["days"].cpu().numpy()
    assert out["log_likelihood"].dtype == torch.float32 and out["days"].dtype == torch.int32
    np.testing.assert_array_equal(days, ref["days"], err_msg=what)
    diff = np.abs(ll - ref["ll"])
    r = _ratio(diff, ref["ll_bound"])
    print(f"{what}: max |ll - ll_ref| / bound = {r:.3e}   (max |ll_ref| = {np.abs(ref['ll']).max():.3e})")
    assert (diff <= ref["ll_bound"]).all(), (what, r)
    gll = out["group_log_likelihood"].double().cpu().numpy()
    have = ~np.isnan(ref["group_ll"])
    assert np.isnan(gll[~have]).all(), what
    assert (np.abs(gll - ref["group_ll"])[have] <= ref["group_ll_bound"][have]).all(), what


def _check_linear(out, ref, G, n_obs, what):
    g = out["policy_gradient"]
    assert g["weight"].dtype == torch.float32 and g["weight"].shape == (G, n_obs) and g["bias"].shape == (G,)
    got = np.concatenate([g["weight"].double().cpu().numpy(), g["bias"].double().cpu().numpy()[:, None]], axis=1)
    want = np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1)
    empty = np.isnan(want).all(axis=1)
    assert np.isnan(got[empty]).all() and np.isfinite(got[~empty]).all(), what  # NaN rows for a group without envs
    diff = np.abs(got - want)[~empty]
    r = _ratio(diff, ref["bound"][~empty])
    print(f"{what}: max |g - g_ref| / bound = {r:.3e}   (max |g_ref| = {np.abs(want[~empty]).max():.3e})")
    assert (diff <= ref["bound"][~empty]).all(), (what, r)
    _check_ll(out, ref, what)
    return got


def _check_mlp(out, ref, layers, what):
    got = [(dW.double().cpu().numpy(), db.double().cpu().numpy()) for dW, db in out["policy_gradient"]["layers"]]
    assert [(a.shape, b.shape) for a, b in got] == [(W.shape, b.shape) for W, b in layers], what
    ratio = 0.0
    for (dW, db), (rW, rb), (bW, bb) in zip(got, ref["layers"], ref["bound"]):
        for x, r, bd in ((dW, rW, bW), (db, rb, bb)):
            assert np.isfinite(x).all() and np.isfinite(r).all(), what
            diff = np.abs(x - r)
            ratio = max(ratio, _ratio(diff, bd))
            assert (diff <= bd).all(), (what, ratio)
    print(f"{what}: max |g - g_ref| / bound = {ratio:.3e}   near-kink fraction {ref['near_kink']:.2e}")
    _check_ll(out, ref, what)
    return got


def _linear_params(ct, G, seed=3, scale=0.4):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((G, ct.n_obs)) * scale).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] *= 0.1
    return W, (rng.standard_normal(G) * 0.5).astype(np.float32)


# name: (table, N, G, rollout_order, prefix days, n_steps, require_budget, schedule, weights, env keywords)
LINEAR = {
    "synth_hindsight_mid_G3": ("synth", 193, 3, False, 9, None, False, "hindsight", "mixed", {}),
    "synth_order_G1": ("synth", 65, 1, True, 9, None, True, "hindsight", None, dict(lockstep=False, rollout_order=True)),
    "synth_one_env": ("synth", 1, 1, False, 0, None, False, "random", None, {}),
    "mini_ones_n17": ("mini", 63, 1, False, 0, 17, False, "ones", None, {}),
    "mini_ones_rb": ("mini", 193, 3, False, 9, None, True, "ones", "mixed", {}),
    "synth_zeros": ("synth", 63, 1, False, 0, 40, False, "zeros", "mixed", {}),
    "ragged_finished_on_entry": ("ragged", 193, 3, False, 25, None, False, "random", "mixed", {}),
    "ragged_hindsight": ("ragged", 65, 1, False, 0, None, True, "hindsight", None, {}),
    "slot27_random_rb": ("slot27", 65, 1, False, 9, None, True, "random", "mixed", {}),
    "ragged27_ones": ("ragged27", 193, 3, False, 0, 30, False, "ones", "mixed", {}),
    "synth_posterior_mean": ("synth", 65, 1, False, 9, None, False, "random", "mixed", dict(reward_mode="posterior_mean")),
}


@pytest.mark.parametrize("case", list(LINEAR))
def test_linear_against_stepped_twin(dev, data, case):
    """N in {1, 63, 65, 193}; G = 1 and G = 3 with group 1 empty (NaN rows); the handle's visiting order set and unset;
    a prefix of days first (t0 > 0, streaks, a non-empty 14-day window); n_steps shorter than the episode; envs
    finished on entry; hindsight, all-zero, all-one (attempts over budget, with and without require_budget) and random
    schedules; weights with zeros and negative values; the ragged and slot-27 tables and reward_mode="posterior_mean",
    which must be accepted."""
    name, n, G, order, prefix, n_steps, rb, sched_kind, wkind, kw = LINEAR[case]
    ct = data[name][0]
    A, B = _make(dev, data, name, n, **kw), _make(dev, data, name, n, **kw)
    if prefix:
        for e_ in (A, B):
            _advance(e_, ct, prefix)
    assert (A._h is not None) and (not order or A.rollout_order)
    st0 = {k: v.cpu().numpy() for k, v in A.state().items()}
    if prefix and name == "synth":
        live = st0["finished"] == 0
        assert (st0["t"][live] > 0).all() and (st0["hist14"][live] != 0).any() and (n == 1 or (st0["streak"][live] > 0).any())
    if case == "ragged_finished_on_entry":
        assert (st0["finished"] != 0).any() and (st0["finished"] == 0).any()
    g = (np.arange(n) % 2 * 2) if G == 3 else None
    W, b = _linear_params(ct, G)
    pol = dict(kind="linear", weight=W, bias=b, require_budget=rb, sample=True, seed=123)  # sample, seed: ignored
    if g is not None:
        pol["group"] = g
    sched = _schedule("random" if (sched_kind == "hindsight" and name not in ("synth", "mini", "ragged")) else sched_kind, A, n, ct.T)
    w = _weights(n, wkind)
    out = A.imitation_gradient(pol, sched, env_weight=w, n_steps=n_steps)
    assert A.check_status() == 0
    S = ct.T if n_steps is None else n_steps
    R, _ = _step_reference(B, sched, S, rb)
    if sched_kind == "ones":
        assert (R["labels"] & R["valid"]).sum() > (st0["budget"] - st0["used"]).clip(min=0).sum()  # attempts over budget
        assert R["forced"].any() == rb
    ref = imitation_linear_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, W, b, g, G)
    _check_linear(out, ref, G, ct.n_obs, case)
    A.close()
    B.close()


@pytest.mark.parametrize("net", list(MATRIX))
def test_mlp_every_instantiation_against_stepped_twin(dev, data, net):
    """The six <WIDTH, LAYERS> instantiations of k_im_pass1 / k_pgm_pass2 with the nets of
    tests/policy_gradient_mlp_cases.py (both activations, one- and two-row outputs, padded units): 193 envs, G = 5
    interleaved groups, a 9-day prefix, hindsight and random schedules and require_budget alternating over the nets."""
    pair, hidden, act, n_out = MATRIX[net]
    assert (policy.mlp_width(hidden), len(hidden)) == pair
    i = list(MATRIX).index(net)
    rb, sched_kind, n = i % 2 == 1, ("hindsight", "random", "ones")[i % 3], 193
    ct = data["synth"][0]
    A, B = _make(dev, data, "synth", n), _make(dev, data, "synth", n)
    for e_ in (A, B):
        e_.rollout(_prefix_policy(ct), n_steps=9)
    g = E.groups(n)
    layers = case_net(ct, net, hidden, n_out)
    pol = dict(kind="mlp", layers=layers, activation=act, group=g, require_budget=rb)
    sched = _schedule(sched_kind, A, n, ct.T)
    w = _weights(n, "mixed")
    out = A.imitation_gradient(pol, sched, env_weight=w)
    assert A.check_status() == 0
    R, _ = _step_reference(B, sched, ct.T, rb)
    ref = imitation_mlp_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, layers, act, g, E.G)
    assert ref["near_kink"] < 0.01
    _check_mlp(out, ref, layers, f"<{pair[0]}, {pair[1]}> {net} rb={rb} {sched_kind}")
    A.close()
    B.close()


def test_mlp_on_table_edges_and_short_calls(dev, data):
    """ragged27 (ragged episode lengths and slot-27 coefficient rows: must be accepted), 65 envs, G = 1 without an
    order, n_steps shorter than the episodes, no weights; and one env."""
    for name, n, n_steps, net in (("ragged27", 65, 30, "tanh7x13"), ("ragged", 1, None, "relu33")):
        _, hidden, act, n_out = MATRIX[net]
        ct = data[name][0]
        A, B = _make(dev, data, name, n), _make(dev, data, name, n)
        layers = [(W[:1], b[:1]) for W, b in case_net(ct, net, hidden, n_out)]
        sched = _schedule("random", A, n, ct.T)
        out = A.imitation_gradient(dict(kind="mlp", layers=layers, activation=act), sched, n_steps=n_steps)
        S = ct.T if n_steps is None else n_steps
        R, _ = _step_reference(B, sched, S, False)
        ref = imitation_mlp_fp64(R["obs"], R["labels"], R["valid"], R["forced"], None, layers, act, None, 1)
        _check_mlp(out, ref, layers, f"{name} {net} n={n}")
        A.close()
        B.close()


def test_mlp_several_tiles_per_wave_and_groups_per_tile(dev, data):
    """65 736 envs on a 12-day table: 1 028 tiles, 2 per wave of the second pass; G = 5 interleaved groups in the
    group-major order, so tiles at the group boundaries hold two groups (the flush on a group change inside a wave). <16, 2>, padded units."""
    n, net = 65_736, "tanh7x13"
    _, hidden, act, n_out = MATRIX[net]
    ct = data["short"][0]
    assert ct.T == 12 and ((n + 63) // 64 + 1023) // 1024 == 2
    A, B = _make(dev, data, "short", n), _make(dev, data, "short", n)
    g = E.groups(n)
    assert ((np.cumsum(np.bincount(g))[:-1] % 64) != 0).any()  # a group boundary falls inside a tile
    layers = case_net(ct, net, hidden, n_out)
    sched = _schedule("random", A, n, ct.T)
    w = _weights(n, "mixed")
    out = A.imitation_gradient(dict(kind="mlp", layers=layers, activation=act, group=g, require_budget=True), sched, env_weight=w)
    R, fin = _step_reference(B, sched, ct.T, True)
    assert bool(fin.all()) and R["forced"].any()
    ref = imitation_mlp_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, layers, act, g, E.G)
    _check_mlp(out, ref, layers, f"2 tiles per wave, {net}")
    A.close()
    B.close()


def _policies(ct, g):
    W, b = _linear_params(ct, 3)
    _, hidden, act, n_out = MATRIX["relu7x29_o2"]
    layers = [(Wl[:3], bl[:3]) for Wl, bl in case_net(ct, "relu7x29_o2", hidden, n_out)]
    return {"linear": dict(kind="linear", weight=W, bias=b, group=g, require_budget=True),
            "mlp": dict(kind="mlp", layers=layers, activation=act, group=g, require_budget=True)}


def _flat(out):
    pg = out["policy_gradient"]
    parts = [pg["weight"], pg["bias"]] if "weight" in pg else [x for pair in pg["layers"] for x in pair]
    return parts + [out["log_likelihood"], out["days"], out["group_log_likelihood"]]


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_no_side_effects_and_identical_bits(dev, data, kind):
    """Two identical calls return identical bits; state(), the observation buffer and a subsequent sampled rollout()
    are bit-identical to those of a twin that never made the call (also mid-episode, after steps)."""
    ct = data["synth"][0]
    n = 193
    A, B = _make(dev, data, "synth", n), _make(dev, data, "synth", n)
    g = np.arange(n) % 3
    pol = _policies(ct, g)[kind]
    sched = _schedule("random", A, n, ct.T)
    w = _weights(n, "mixed")
    for e_ in (A, B):
        for _ in range(3):
            e_.step(sched[:, 0].to(torch.int32))
    o1 = A.imitation_gradient(pol, sched, env_weight=w)
    o2 = A.imitation_gradient(pol, sched, env_weight=w)
    for x, y in zip(_flat(o1), _flat(o2)):
        assert torch.equal(x.nan_to_num(7.0) if x.is_floating_point() else x, y.nan_to_num(7.0) if y.is_floating_point() else y)
    sa, sb = A.state(), B.state()
    for k in sb:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(A._obs, B._obs) and A.check_status() == 0
    roll = dict(_policies(ct, g)["linear"], sample=True, seed=6)
    ra, rb_ = A.rollout(roll, alert_mask=True), B.rollout(roll, alert_mask=True)
    assert set(ra) == set(rb_)
    for k, v in rb_.items():
        assert torch.equal(ra[k].nan_to_num(7.0) if v.is_floating_point() else ra[k], v.nan_to_num(7.0) if v.is_floating_point() else v), k
    assert torch.equal(A._obs, B._obs)
    A.close()
    B.close()


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_split_stretch_adds_up(dev, data, kind):
    """k days, step() along the schedule for k days, then the other S - k days (env_weight zeroed for envs that
    finished in between: step() goes on shifting their history): the two gradients add up to the whole stretch's
    within the sum of the two calls' bounds, each taken from the restatement on its own days of the stepped twin."""
    name, n, k, S = "ragged", 193, 23, 60
    ct = data[name][0]
    A, B, T_ = (_make(dev, data, name, n) for _ in range(3))
    g = np.arange(n) % 3
    pol = dict(_policies(ct, g)[kind], require_budget=False)
    sched = _schedule("random", A, n, ct.T)
    w = _weights(n, "mixed")
    whole = A.imitation_gradient(pol, sched, env_weight=w, n_steps=S)
    first = B.imitation_gradient(pol, sched, env_weight=w, n_steps=k)
    _, fin = _step_reference(B, sched, k, False)
    assert bool(fin.any()) and not bool(fin.all())
    w2 = np.where(fin.cpu().numpy(), np.float32(0.0), w)
    second = B.imitation_gradient(pol, sched, env_weight=w2, n_steps=S - k)
    R, _ = _step_reference(T_, sched, S, False)
    halves = []
    for lo, hi, ww in ((0, k, w), (k, S, w2)):
        sl = {kk: v[lo:hi] for kk, v in R.items()}
        if kind == "linear":
            ref = imitation_linear_fp64(sl["obs"], sl["labels"], sl["valid"], sl["forced"], ww, pol["weight"], pol["bias"], g, 3)
            halves.append([ref["bound"][:, :-1], ref["bound"][:, -1]])
        else:
            ref = imitation_mlp_fp64(sl["obs"], sl["labels"], sl["valid"], sl["forced"], ww, pol["layers"], pol["activation"], g, 3)
            halves.append([x for pair in ref["bound"] for x in pair])
    npar = len(halves[0])
    worst = 0.0
    for x, a, b_, b1, b2 in zip(_flat(whole)[:npar], _flat(first)[:npar], _flat(second)[:npar], *halves):
        diff = np.abs(x.double().cpu().numpy() - a.double().cpu().numpy() - b_.double().cpu().numpy())
        worst = max(worst, _ratio(diff, b1 + b2))
        assert (diff <= b1 + b2).all(), (kind, worst)
    print(f"split {kind}: max |whole - (first + second)| / (bound1 + bound2) = {worst:.3e}")
    lw = whole["log_likelihood"].double()
    torch.testing.assert_close(lw, first["log_likelihood"].double() + second["log_likelihood"].double(), rtol=1e-6, atol=1e-6)
    assert torch.equal(whole["days"], first["days"] + second["days"])
    for e_ in (A, B, T_):
        e_.close()


def test_refusals(dev, data):
    """A stale observation buffer (after load_state_dict) is a RuntimeError; bad arguments are ValueErrors before
    anything runs: the state is untouched."""
    ct = data["synth"][0]
    n = 65
    env = _make(dev, data, "synth", n)
    W, b = _linear_params(ct, 1)
    lin = dict(kind="linear", weight=W, bias=b)
    sched = _schedule("random", env, n, ct.T)
    before = {k: v.clone() for k, v in env.state().items()}
    for pol, kw in (({"kind": "never"}, {}), (lin, dict(n_steps=0)), (lin, dict(env_weight=np.full(n, np.nan))),
                    (lin, dict(env_weight=np.ones(n + 1))), (dict(lin, weight=W[:, :-1]), {})):
        with pytest.raises(ValueError):
            env.imitation_gradient(pol, sched, **kw)
    for bad in (sched[:, :-1], sched.to(torch.uint8), sched[:-1]):
        with pytest.raises(ValueError):
            env.imitation_gradient(lin, bad)
    for k_, v in env.state().items():
        assert torch.equal(v, before[k_]), k_
    env.imitation_gradient(lin, sched, n_steps=3)
    env.load_state_dict(env.state_dict())
    with pytest.raises(RuntimeError):
        env.imitation_gradient(lin, sched)
    env.close()
    fx = _make(dev, data, "synth", n, fixes=["lag"])
    with pytest.raises(ValueError):
        fx.imitation_gradient(lin, sched)
    fx.close()
