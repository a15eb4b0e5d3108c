"""value_gradient() (k_value_gradient_linear; k_vg_pass1 + k_vg_finish + the second pass of w2a_policy_gradient_mlp) and
imitation_gradient(day_weight=...) against the fp64 restatement (tests/value_gradient_restatement.py). The reference
never touches the kernels under test: an identical twin from the same seed is stepped day by day through step() along
the schedule, every env read on its own days only, and the rows and rewards it returns go to the restatement. Every
comparison requires |x - x_ref| <= bound for every component and prints the largest ratio to the bound."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obs_layouts as L  # noqa: E402
import table_edges as E  # noqa: E402
from policy_gradient_mlp_cases import MATRIX, net as case_net  # noqa: E402
from policy_gradient_mlp_restatement import policy_gradient_mlp_fp64  # noqa: E402
from policy_gradient_restatement import policy_gradient_fp64  # noqa: E402
from value_gradient_restatement import (value_linear_fp64, value_mlp_fp64, weighted_imitation_linear_fp64,  # noqa: E402
                                        weighted_imitation_mlp_fp64)

from weather2alert_amd import policy, synth, tables  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RETURN_RTOL, RETURN_ATOL = 2e-6, 2e-5  # as tests/test_env_gpu.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def data():
    """name -> (compiled tables, env keywords, reset seed, reset options)"""
    sd = synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=6, seed=17, extra_confounder_fips=3)
    out = {"synth": (tables.compile_from_synth(sd), dict(similar_climate_counties=True), 5, {"budget": 10})}
    for name, tb in E.make_tables().items():
        out[name] = (tb.ct, dict(similar_climate_counties=True), E.RESET[name]["seed"], dict(E.RESET[name]["opts"]))
    tb = L.make_table("n8")
    out["n8"] = (tb.ct, dict(similar_climate_counties=True), L.RESET["n8"]["seed"], dict(L.RESET["n8"]["opts"]))
    return out


def _make(dev, data, name, n, **kw):
    from weather2alert_amd import HeatAlertVecEnv

    ct, ekw, seed, opts = data[name]
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=E.GID0, **{**ekw, **kw})
    env.reset(seed=seed, options=dict(opts))
    return env


def _sampled_policy(ct, bias=0.3, seed=4, require_budget=False):
    """a sampled linear policy that alerts often: streaks, a non-empty 14-day window, and budgets that run out"""
    rng = np.random.default_rng(9)
    W = (rng.standard_normal((1, ct.n_obs)) * 0.2).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] *= 0.1
    return dict(kind="linear", weight=W, bias=np.array([bias], np.float32), sample=True, seed=seed,
                require_budget=require_budget)


def _step_reference(env, sched, S, require_budget=False):
    """`env` stepped through step() along `sched` (attempts by day of the episode) for at most S days from where it
    stands; every env is read on its own days only. Returns numpy obs f64 [S, n, n_obs] (the row held before decision
    s), reward f64, labels / valid / forced bool [S, n]."""
    n, dv = env.num_envs, env.device
    rows = torch.arange(n, device=dv)
    fin = env.state()["finished"].bool()
    R = dict(obs=torch.zeros((S, n, env._obs.shape[1]), dtype=torch.float64, device=dv),
             reward=torch.zeros((S, n), dtype=torch.float64, device=dv),
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
        res = env.step((R["labels"][s] & ~R["forced"][s]).to(torch.int32))
        R["reward"][s] = torch.where(~fin, res[1].double(), torch.zeros_like(R["reward"][s]))
        fin = fin | res[2].bool()
    return {k: v.cpu().numpy() for k, v in R.items()}


def _ratio(diff, bound):
    return float(np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0)).max())


def _within(got, want, bound, what, label):
    diff = np.abs(got - want)
    r = _ratio(diff, bound)
    print(f"{what}: max |{label} - ref| / bound = {r:.3e}   (max |ref| = {np.abs(want).max():.3e})")
    assert (diff <= bound).all(), (what, label, r)


def _check_per_env(out, ref, S, what, advantage=True):
    assert out["sq_error"].dtype == torch.float32 and out["days"].dtype == torch.int32 and out["return"].dtype == torch.float32
    np.testing.assert_array_equal(out["days"].cpu().numpy(), ref["days"], err_msg=what)
    _within(out["sq_error"].double().cpu().numpy(), ref["sq"], ref["sq_bound"], what, "sq_error")
    _within(out["return"].double().cpu().numpy(), ref["ret"], ref["ret_bound"], what, "return")
    if advantage:
        adv = out["advantage"]
        assert adv.dtype == torch.float32 and tuple(adv.shape) == (S, ref["days"].shape[0])
        a = adv.double().cpu().numpy()
        valid = ref["adv_bound"] > 0
        assert (a[:ref["advantage"].shape[0]][~valid] == 0).all() and (a[ref["advantage"].shape[0]:] == 0).all(), what
        _within(a[:ref["advantage"].shape[0]], ref["advantage"], ref["adv_bound"], what, "advantage")
    else:
        assert "advantage" not in out
    gl = out["group_loss"].double().cpu().numpy()
    have = ~np.isnan(ref["group_loss"])
    assert np.isnan(gl[~have]).all(), what
    _within(gl[have], ref["group_loss"][have], ref["group_loss_bound"][have], what, "group_loss")


def _check_linear(out, key, ref, G, n_obs, what):
    g = out[key]
    assert g["weight"].dtype == torch.float32 and g["weight"].shape == (G, n_obs) and g["bias"].shape == (G,)
    got = np.concatenate([g["weight"].double().cpu().numpy(), g["bias"].double().cpu().numpy()[:, None]], axis=1)
    want = np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1)
    empty = np.isnan(want).all(axis=1)
    assert np.isnan(got[empty]).all() and np.isfinite(got[~empty]).all(), what  # NaN rows for a group without envs
    _within(got[~empty], want[~empty], ref["bound"][~empty], what, "g")
    return got


def _check_mlp(out, key, ref, layers, what, empty=()):
    got = [(dW.double().cpu().numpy(), db.double().cpu().numpy()) for dW, db in out[key]["layers"]]
    assert [(a.shape, b.shape) for a, b in got] == [(np.asarray(W).shape, np.asarray(b).shape) for W, b in layers], what
    keep = np.array([k not in empty for k in range(got[0][0].shape[0])])
    ratio = 0.0
    for (dW, db), (rW, rb), (bW, bb) in zip(got, ref["layers"], ref["bound"]):
        for x, r, bd in ((dW, rW, bW), (db, rb, bb)):
            assert np.isnan(x[~keep]).all() and np.isfinite(x[keep]).all() and np.isfinite(r[keep]).all(), what
            diff = np.abs(x - r)[keep]
            ratio = max(ratio, _ratio(diff, bd[keep]))
            assert (diff <= bd[keep]).all(), (what, ratio)
    print(f"{what}: max |g - g_ref| / bound = {ratio:.3e}   near-kink fraction {ref['near_kink']:.2e}")
    return got


def _linear_params(ct, G, seed=3, scale=0.4):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((G, ct.n_obs)) * scale).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] *= 0.1
    return W, (rng.standard_normal(G) * 0.5).astype(np.float32)


def _weights(n):
    w = np.random.default_rng(8).standard_normal(n).astype(np.float32)  # negative values
    w[::5] = 0.0
    return w


G4 = 4  # groups 0, 1 and 3 hold envs, group 2 is empty: a NaN block


def _groups4(n):
    return np.array([0, 1, 3])[np.arange(n) % 3]


def _net4(ct, name):
    _, hidden, act, n_out = MATRIX[name]
    layers = case_net(ct, name, hidden, n_out)
    assert layers[0][0].shape[0] >= G4
    return [(W[:G4], b[:G4]) for W, b in layers], act


BASE = [("linear", 1, "hindsight"), ("linear", 3, "attempts"), ("linear", None, "hindsight"), ("linear", None, "rollout"),
        ("mlp", 1, "rollout"), ("mlp", 3, "hindsight"), ("mlp", None, "hindsight"), ("mlp", None, "attempts")]


@pytest.mark.parametrize("kind,n_steps,sched_kind", BASE)
def test_against_stepped_twin(dev, data, kind, n_steps, sched_kind):
    """300 envs (four full waves and a partial one) on the ragged table after a 25-day prefix (t0 > 0, streaks, a
    non-empty 14-day window, some envs finished on entry), G = 3 groups with envs plus one empty group (a NaN block),
    n_steps in {1, 3, the rest of the episode}, mixed weights; schedules from hindsight_optimum(), from a sampled
    rollout's alert_days that uses up budgets, and from its attempt_days (attempts over budget)."""
    n, name = 300, "ragged"
    ct = data[name][0]
    A, B, C_ = (_make(dev, data, name, n) for _ in range(3))
    for e_ in (A, B, C_):
        e_.rollout(_sampled_policy(ct), n_steps=25)
    st0 = {k: v.cpu().numpy() for k, v in A.state().items()}
    assert (st0["finished"] != 0).any() and (st0["finished"] == 0).any()
    if sched_kind == "hindsight":
        sched = A.hindsight_optimum()["alert_days"]
    else:
        ro = C_.rollout(_sampled_policy(ct, bias=1.5, seed=7), alert_mask=True)
        assert bool((C_.state()["used"] == C_.state()["budget"]).any())  # budgets used up
        assert bool((ro["attempt_days"] & ~ro["alert_days"]).any())     # and attempts beyond them
        sched = ro["alert_days"] if sched_kind == "rollout" else ro["attempt_days"]
    g, w = _groups4(n), _weights(n)
    what = f"{kind} n_steps={n_steps} {sched_kind}"
    if kind == "linear":
        W, b = _linear_params(ct, G4)
        val = dict(kind="linear", weight=W, bias=b, group=g, sample=True, seed=3, require_budget=True)  # all three ignored
    else:
        layers, act = _net4(ct, "tanh29x9")
        val = dict(kind="mlp", layers=layers, activation=act, group=g)
    out = A.value_gradient(val, sched, env_weight=w, n_steps=n_steps, advantage=True)
    assert A.check_status() == 0
    S = ct.T if n_steps is None else n_steps
    R = _step_reference(B, sched, S)
    if sched_kind == "attempts":
        used_up = (R["labels"].sum(axis=0) > (st0["budget"] - st0["used"]).clip(min=0)) & (st0["finished"] == 0)
        assert used_up.any() or n_steps is not None
    if kind == "linear":
        ref = value_linear_fp64(R["obs"], R["valid"], R["reward"], w, W, b, g, G4)
        _check_linear(out, "value_gradient", ref, G4, ct.n_obs, what)
    else:
        ref = value_mlp_fp64(R["obs"], R["valid"], R["reward"], w, layers, act, g, G4)
        _check_mlp(out, "value_gradient", ref, layers, what, empty=(2,))
    _check_per_env(out, ref, S, what)
    plain = A.value_gradient(val, sched, env_weight=w, n_steps=n_steps)  # advantage off: the same numbers, no rows
    assert "advantage" not in plain
    for k in ("sq_error", "days", "return", "group_loss"):
        assert torch.equal(plain[k].nan_to_num(7.0) if plain[k].is_floating_point() else plain[k],
                           out[k].nan_to_num(7.0) if out[k].is_floating_point() else out[k]), k
    for e_ in (A, B, C_):
        e_.close()


@pytest.mark.parametrize("net", list(MATRIX))
def test_mlp_every_instantiation_against_stepped_twin(dev, data, net):
    """The six <WIDTH, LAYERS> instantiations of k_vg_pass1 / k_pgm_pass2 with the nets of
    tests/policy_gradient_mlp_cases.py (both activations, one- and two-row outputs, padded units): 193 envs, G = 5
    interleaved groups, a 9-day prefix, whole episodes, a random schedule with attempts over budget."""
    pair, hidden, act, n_out = MATRIX[net]
    assert (policy.mlp_width(hidden), len(hidden)) == pair
    n = 193
    ct = data["synth"][0]
    A, B = _make(dev, data, "synth", n), _make(dev, data, "synth", n)
    for e_ in (A, B):
        e_.rollout(_sampled_policy(ct), n_steps=9)
    g = E.groups(n)
    layers = case_net(ct, net, hidden, n_out)
    sched = torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev)
    w = _weights(n)
    out = A.value_gradient(dict(kind="mlp", layers=layers, activation=act, group=g), sched, env_weight=w, advantage=True)
    assert A.check_status() == 0
    R = _step_reference(B, sched, ct.T)
    ref = value_mlp_fp64(R["obs"], R["valid"], R["reward"], w, layers, act, g, E.G)
    assert ref["near_kink"] < 0.01
    what = f"<{pair[0]}, {pair[1]}> {net}"
    _check_mlp(out, "value_gradient", ref, layers, what)
    _check_per_env(out, ref, ct.T, what)
    A.close()
    B.close()


EDGES = [("ragged27", "linear", 30), ("ragged27", "tanh7x13", None), ("slot27", "linear", None), ("slot27", "relu33", 30),
         ("n8", "linear", None), ("n8", "tanh7x13", None)]


@pytest.mark.parametrize("name,kind,n_steps", EDGES)
def test_table_edges_and_another_layout(dev, data, name, kind, n_steps):
    """ragged episode lengths with slot-27 coefficient rows, a slot-27 table (both must be accepted: the rewards' 14-day
    window enters), and the n8 layout of tests/obs_layouts.py (8 observation columns, run-time columns interleaved with
    a table column, slots 4..23 empty): 65 envs, G = 1 without an order, no weights."""
    n = 65
    ct = data[name][0]
    A, B = _make(dev, data, name, n), _make(dev, data, name, n)
    sched = torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev)
    S = ct.T if n_steps is None else n_steps
    what = f"{name} {kind} n_steps={n_steps}"
    if kind == "linear":
        W, b = _linear_params(ct, 1)
        out = A.value_gradient(dict(kind="linear", weight=W, bias=b), sched, n_steps=n_steps, advantage=True)
        R = _step_reference(B, sched, S)
        ref = value_linear_fp64(R["obs"], R["valid"], R["reward"], None, W, b, None, 1)
        _check_linear(out, "value_gradient", ref, 1, ct.n_obs, what)
    else:
        _, hidden, act, n_out = MATRIX[kind]
        layers = [(W[:1], b[:1]) for W, b in case_net(ct, kind, hidden, n_out)]
        out = A.value_gradient(dict(kind="mlp", layers=layers, activation=act), sched, n_steps=n_steps, advantage=True)
        R = _step_reference(B, sched, S)
        ref = value_mlp_fp64(R["obs"], R["valid"], R["reward"], None, layers, act, None, 1)
        _check_mlp(out, "value_gradient", ref, layers, what)
    _check_per_env(out, ref, S, what)
    A.close()
    B.close()


def _values(ct, g):
    W, b = _linear_params(ct, 3)
    _, hidden, act, n_out = MATRIX["relu7x29_o2"]
    layers = [(Wl[:3], bl[:3]) for Wl, bl in case_net(ct, "relu7x29_o2", hidden, n_out)]
    return {"linear": dict(kind="linear", weight=W, bias=b, group=g), "mlp": dict(kind="mlp", layers=layers, activation=act, group=g)}


def _flat(out, key="value_gradient"):
    pg = out[key]
    parts = [pg["weight"], pg["bias"]] if "weight" in pg else [x for pair in pg["layers"] for x in pair]
    return parts + [out[k] for k in ("sq_error", "days", "return", "group_loss", "advantage") if k in out]


def _same(x, y):
    return torch.equal(x.nan_to_num(7.0) if x.is_floating_point() else x, y.nan_to_num(7.0) if y.is_floating_point() else y)


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_no_side_effects_and_identical_bits(dev, data, kind):
    """Two identical calls return identical bits; state(), the observation buffer and a subsequent sampled rollout()
    (the RNG) are bit-identical to those of a twin that never made the call (mid-episode, after steps)."""
    ct = data["synth"][0]
    n = 193
    A, B = _make(dev, data, "synth", n), _make(dev, data, "synth", n)
    g = np.arange(n) % 3
    val = _values(ct, g)[kind]
    sched = torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev)
    w = _weights(n)
    for e_ in (A, B):
        for _ in range(3):
            e_.step(sched[:, 0].to(torch.int32))
    o1 = A.value_gradient(val, sched, env_weight=w, advantage=True)
    o2 = A.value_gradient(val, sched, env_weight=w, advantage=True)
    for x, y in zip(_flat(o1), _flat(o2)):
        assert _same(x, y)
    sa, sb = A.state(), B.state()
    for k in sb:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(A._obs, B._obs) and A.check_status() == 0
    roll = dict(_values(ct, g)["linear"], sample=True, seed=6)
    ra, rb_ = A.rollout(roll, alert_mask=True), B.rollout(roll, alert_mask=True)
    assert set(ra) == set(rb_)
    for k, v in rb_.items():
        assert _same(ra[k], v), k
    assert torch.equal(A._obs, B._obs)
    A.close()
    B.close()


def test_linear_per_env_outputs_do_not_depend_on_groups_or_order(dev, data):
    """sq_error, return, days and advantage of an env are the same bits with one group or three that share a parameter
    row, and with the handle's feature-row visiting order set or unset; with one group the gradient too."""
    ct = data["synth"][0]
    n = 193
    W, b = _linear_params(ct, 1)
    sched = torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev)
    outs = []
    for kw, G in (({}, 1), ({}, 3), (dict(lockstep=False, rollout_order=True), 1)):
        env = _make(dev, data, "synth", n, **kw)
        env.rollout(_sampled_policy(ct), n_steps=9)
        val = dict(kind="linear", weight=np.repeat(W, G, axis=0), bias=np.repeat(b, G))
        if G > 1:
            val["group"] = np.arange(n) % G
        assert not kw or env.rollout_order
        outs.append(env.value_gradient(val, sched, n_steps=60, advantage=True))
        env.close()
    for o in outs[1:]:
        for k in ("sq_error", "return", "days", "advantage"):
            assert torch.equal(o[k], outs[0][k]), k
    for x, y in zip(_flat(outs[0])[:2], _flat(outs[2])[:2]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_zero_critic_advantage_turns_imitation_into_the_policy_gradient(dev, data, kind):
    """An all-zero critic makes "advantage" the reward-to-go Q_s. With require_budget=True, teacher forcing along the
    schedule a sampled rollout issued, weighted by that advantage, is the rollout's own REINFORCE gradient
    (policy_gradient="none"): within the sum of the two derived bounds. "return" is the rollout's, within the suite's
    return bar."""
    n, name = 193, "synth"
    ct = data[name][0]
    A, B, C_ = (_make(dev, data, name, n) for _ in range(3))
    for e_ in (A, B, C_):
        e_.rollout(_sampled_policy(ct), n_steps=9)
    g = np.arange(n) % 3
    if kind == "linear":
        W, b = _linear_params(ct, 3, scale=0.2)
        actor = dict(kind="linear", weight=W, bias=b, group=g, sample=True, seed=11, require_budget=True)
    else:
        _, hidden, act, n_out = MATRIX["tanh7x13"]
        layers = [(Wl[:3], bl[:3]) for Wl, bl in case_net(ct, "tanh7x13", hidden, n_out)]
        actor = dict(kind="mlp", layers=layers, activation=act, group=g, sample=True, seed=11, require_budget=True)
    ro = A.rollout(actor, alert_mask=True, policy_gradient="none")
    assert bool(ro["alert_days"].any()) and torch.equal(ro["attempt_days"], ro["alert_days"])  # attempts = issued alerts
    sched = ro["alert_days"]
    zero = dict(kind="linear", weight=np.zeros((1, ct.n_obs), np.float32), bias=np.zeros(1, np.float32))
    vg = B.value_gradient(zero, sched, advantage=True)
    torch.testing.assert_close(vg["return"], ro["return"], rtol=RETURN_RTOL, atol=RETURN_ATOL)
    im = B.imitation_gradient(actor, sched, day_weight=vg["advantage"])
    R = _step_reference(C_, sched, ct.T, require_budget=True)
    # under require_budget every scored day's attempt is the alert issued: the labels are the policy's own draws there
    Q = np.cumsum(np.where(R["valid"], R["reward"], 0.0)[::-1], axis=0)[::-1]
    what = f"cross-check {kind}"
    if kind == "linear":
        pg = policy_gradient_fp64(R["obs"], R["labels"], R["valid"], R["forced"], R["reward"], None, W, b, g, 3)
        wi = weighted_imitation_linear_fp64(R["obs"], R["labels"], R["valid"], R["forced"], None, Q, W, b, g, 3)
        got_im = np.concatenate([im["policy_gradient"]["weight"].double().cpu().numpy(), im["policy_gradient"]["bias"].double().cpu().numpy()[:, None]], axis=1)
        got_pg = np.concatenate([ro["policy_gradient"]["weight"].double().cpu().numpy(), ro["policy_gradient"]["bias"].double().cpu().numpy()[:, None]], axis=1)
        _within(got_im, got_pg, pg["bound"] + wi["bound"], what, "imitation(day_weight=advantage) vs policy_gradient")
        _within(got_im, np.concatenate([wi["weight"], wi["bias"][:, None]], axis=1), wi["bound"] + pg["bound"], what, "imitation vs restatement")
    else:
        pg = policy_gradient_mlp_fp64(R["obs"], R["labels"], R["valid"], R["forced"], R["reward"], None, layers, act, g, 3)
        wi = weighted_imitation_mlp_fp64(R["obs"], R["labels"], R["valid"], R["forced"], None, Q, layers, act, g, 3)
        worst = 0.0
        for (iW, ib), (pW, pb), (b1W, b1b), (b2W, b2b) in zip(im["policy_gradient"]["layers"], ro["policy_gradient"]["layers"], pg["bound"], wi["bound"]):
            for x, y, bd in ((iW, pW, b1W + b2W), (ib, pb, b1b + b2b)):
                diff = np.abs(x.double().cpu().numpy() - y.double().cpu().numpy())
                worst = max(worst, _ratio(diff, bd))
                assert (diff <= bd).all(), (what, worst)
        print(f"{what}: max |imitation(day_weight=advantage) - policy_gradient| / (bound1 + bound2) = {worst:.3e}")
    for e_ in (A, B, C_):
        e_.close()


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_day_weight_against_stepped_twin(dev, data, kind):
    """Random day weights [S + 2, N] (more call-days than the call runs) by call-day and env id, after a 9-day prefix
    (call-day != day of the episode) and with three interleaved groups (env id != visiting position for the MLP kind),
    next to env weights; None is bit-identical to the call without the argument and, for the linear kind, to ones."""
    n, name, S = 193, "synth", 40
    ct = data[name][0]
    A, B = _make(dev, data, name, n), _make(dev, data, name, n)
    for e_ in (A, B):
        e_.rollout(_sampled_policy(ct), n_steps=9)
    g = np.arange(n) % 3
    sched = torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev)
    w = _weights(n)
    dw = np.random.default_rng(5).standard_normal((S + 2, n)).astype(np.float32)
    if kind == "linear":
        W, b = _linear_params(ct, 3)
        pol = dict(kind="linear", weight=W, bias=b, group=g, require_budget=True)
    else:
        _, hidden, act, n_out = MATRIX["relu7x29_o2"]
        layers = [(Wl[:3], bl[:3]) for Wl, bl in case_net(ct, "relu7x29_o2", hidden, n_out)]
        pol = dict(kind="mlp", layers=layers, activation=act, group=g, require_budget=True)
    out = A.imitation_gradient(pol, sched, env_weight=w, n_steps=S, day_weight=torch.as_tensor(dw, device=dev))
    base = A.imitation_gradient(pol, sched, env_weight=w, n_steps=S)
    none = A.imitation_gradient(pol, sched, env_weight=w, n_steps=S, day_weight=None)
    ones = A.imitation_gradient(pol, sched, env_weight=w, n_steps=S, day_weight=torch.ones((S, n), device=dev))
    npar = 2 if kind == "linear" else 2 * len(pol["layers"])
    fl = lambda o: _flat(o, "policy_gradient")[:npar] + [o["log_likelihood"], o["days"]]  # noqa: E731
    for x, y in zip(fl(base), fl(none)):
        assert _same(x, y)
    if kind == "linear":
        for x, y in zip(fl(base), fl(ones)):
            assert _same(x, y)
    for k in ("log_likelihood", "days"):
        assert torch.equal(out[k], base[k]), k
    R = _step_reference(B, sched, S, require_budget=True)
    what = f"day_weight {kind}"
    if kind == "linear":
        ref = weighted_imitation_linear_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, dw, W, b, g, 3)
        _check_linear(out, "policy_gradient", ref, 3, ct.n_obs, what)
    else:
        ref = weighted_imitation_mlp_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, dw, layers, act, g, 3)
        _check_mlp(out, "policy_gradient", ref, layers, what)
    A.close()
    B.close()


def test_refusals(dev, data):
    """A stale observation buffer (after load_state_dict) is a RuntimeError; bad arguments, reward modes and semantics
    are ValueErrors before anything runs: the state is untouched."""
    ct = data["synth"][0]
    n = 65
    env = _make(dev, data, "synth", n)
    W, b = _linear_params(ct, 1)
    lin = dict(kind="linear", weight=W, bias=b)
    sched = torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev)
    before = {k: v.clone() for k, v in env.state().items()}
    obs_before = env._obs.clone()
    for val, kw in (({"kind": "never"}, {}), ({"kind": "bernoulli", "p": 0.1}, {}), (lin, dict(n_steps=0)),
                    (lin, dict(env_weight=np.full(n, np.nan))), (lin, dict(env_weight=np.ones(n + 1))),
                    (dict(lin, weight=W[:, :-1]), {})):
        with pytest.raises(ValueError):
            env.value_gradient(val, sched, **kw)
    for bad in (sched[:, :-1], sched.to(torch.uint8), sched[:-1]):
        with pytest.raises(ValueError):
            env.value_gradient(lin, bad)
    for dw in (torch.ones((2, n), device=dev), torch.ones((3, n + 1), device=dev), torch.ones((3, n), device=dev, dtype=torch.int32)):
        with pytest.raises(ValueError):
            env.imitation_gradient(lin, sched, n_steps=3, day_weight=dw)
    for k_, v in env.state().items():
        assert torch.equal(v, before[k_]), k_
    assert torch.equal(env._obs, obs_before)
    env.value_gradient(lin, sched, n_steps=3)
    env.load_state_dict(env.state_dict())
    with pytest.raises(RuntimeError):
        env.value_gradient(lin, sched)
    env.close()
    for kw in (dict(fixes=["lag"]), dict(reward_mode="posterior_mean")):
        fx = _make(dev, data, "synth", n, **kw)
        with pytest.raises(ValueError):
            fx.value_gradient(lin, sched)
        fx.close()
