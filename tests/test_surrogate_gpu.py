"""surrogate_gradient() (k_surrogate_linear; k_sg_pass1 + the second pass of w2a_policy_gradient_mlp) against the fp64
restatement (tests/surrogate_restatement.py). The reference never touches the kernels under test: an identical twin from
the same seed is stepped day by day through step() with the schedule's actions (tests/test_imitation_gpu.py's
_step_reference) and the rows it returns go to the restatement. old_log_prob is the "log_prob" output of the same entry
point for a perturbed copy of the policy -- an input both sides read -- and that output is itself held to the
restatement's log pi. Every comparison requires |got - ref| <= bound for every component of the gradient, the surrogate,
approx_kl, the entropy, the log-probabilities and the group means, equal day counts, clipped_days equal up to the env's
ambiguous days, at most 1 % ambiguous days, and prints the largest ratio to the bound.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obs_layouts as L  # noqa: E402
import table_edges as E  # noqa: E402
from imitation_restatement import imitation_linear_fp64, imitation_mlp_fp64  # noqa: E402
from policy_gradient_mlp_cases import MATRIX, net as case_net  # noqa: E402
from surrogate_restatement import AMBIGUOUS_CAP, surrogate_linear_fp64, surrogate_mlp_fp64  # noqa: E402
from test_imitation_gpu import (_advance, _linear_params, _make, _prefix_policy, _ratio, _schedule,  # noqa: E402,F401
                                _step_reference, _weights, data, dev)
from value_gradient_restatement import weighted_imitation_linear_fp64, weighted_imitation_mlp_fp64  # noqa: E402

pytestmark = pytest.mark.gpu

N, G = 300, 4  # 4 full waves and a partial one; groups 0, 1, 3 and the empty group 2
CLIP = 0.2


def _groups(n):
    return np.array([0, 1, 3])[np.arange(n) % 3]


def _advantage(S, n, seed=31):
    """both signs, zeros, magnitudes around 1"""
    A = np.random.default_rng(seed).standard_normal((S, n)).astype(np.float32)
    A[:, ::11] = 0.0
    return A


def _perturb(arrays, seed, size=0.3):
    rng = np.random.default_rng(seed)
    return [(x + size * np.abs(x).mean() * rng.standard_normal(x.shape)).astype(np.float32) for x in arrays]


def _perturbed_policy(pol, seed=77):
    if pol["kind"] == "linear":
        W, b = _perturb([pol["weight"], pol["bias"]], seed)
        return dict(pol, weight=W, bias=b)
    Ws, bs = _perturb([W for W, _ in pol["layers"]], seed), _perturb([b for _, b in pol["layers"]], seed + 1)
    return dict(pol, layers=list(zip(Ws, bs)))


def _restate(pol, R, w, A, old, clip, beta, g, n_groups):
    args = (R["obs"], R["labels"], R["valid"], R["forced"], w, A, old, clip, beta)
    if pol["kind"] == "linear":
        return surrogate_linear_fp64(*args, pol["weight"], pol["bias"], g, n_groups)
    return surrogate_mlp_fp64(*args, pol["layers"], pol["activation"], g, n_groups)


def _grad_parts(out, ref, pol):
    """[(got, want, bound), ...] over the parameter arrays"""
    pg = out["policy_gradient"]
    if pol["kind"] == "linear":
        got = np.concatenate([pg["weight"].double().cpu().numpy(), pg["bias"].double().cpu().numpy()[:, None]], axis=1)
        return [(got, np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1), ref["bound"])]
    parts = []
    assert [(a.shape, b.shape) for a, b in pg["layers"]] == [(W.shape, b.shape) for W, b in pol["layers"]]
    for (dW, db), (rW, rb), (bW, bb) in zip(pg["layers"], ref["layers"], ref["bound"]):
        parts += [(dW.double().cpu().numpy(), rW, bW), (db.double().cpu().numpy(), rb, bb)]
    return parts


def _check(out, ref, pol, what, log_prob=None):
    """every component within its bound; returns the largest ratio to the bound"""
    assert ref["ambiguous_share"] <= AMBIGUOUS_CAP, (what, ref["ambiguous_share"])
    worst = {}
    for got, want, bound in _grad_parts(out, ref, pol):
        empty = np.isnan(want)
        assert np.isnan(got[empty]).all() and np.isfinite(got[~empty]).all(), what  # NaN for a group without envs
        diff = np.abs(got - want)[~empty]
        worst["gradient"] = max(worst.get("gradient", 0.0), _ratio(diff, bound[~empty]))
        assert (diff <= bound[~empty]).all(), (what, "gradient", worst)
    for key, name in (("surrogate", "L"), ("approx_kl", "kl"), ("entropy", "H")):
        assert out[key].dtype == torch.float32
        diff = np.abs(out[key].double().cpu().numpy() - ref[name])
        worst[key] = _ratio(diff, ref[name + "_bound"])
        assert (diff <= ref[name + "_bound"]).all(), (what, key, worst)
    assert out["days"].dtype == torch.int32 and out["clipped_days"].dtype == torch.int32
    np.testing.assert_array_equal(out["days"].cpu().numpy(), ref["days"], err_msg=what)
    assert (np.abs(out["clipped_days"].cpu().numpy() - ref["clipped"]) <= ref["clipped_tol"]).all(), what
    gs = out["group_surrogate"].double().cpu().numpy()
    have = ~np.isnan(ref["group_surrogate"])
    assert np.isnan(gs[~have]).all(), what
    assert (np.abs(gs - ref["group_surrogate"])[have] <= ref["group_surrogate_bound"][have]).all(), what
    lp = out.get("log_prob") if log_prob is None else log_prob
    if lp is not None:
        lp = lp.double().cpu().numpy()
        assert lp.shape == ref["lp"].shape and (lp[~ref["m"]] == 0).all(), what  # zero where the env does not score
        diff = np.abs(lp - ref["lp"])
        worst["log_prob"] = _ratio(diff, ref["lp_bound"])
        assert (diff <= ref["lp_bound"]).all(), (what, "log_prob", worst)
    print(f"{what}: ratio to the bound " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items())
          + f"; ambiguous share {ref['ambiguous_share']:.2e}, clipped {int(ref['clipped'].sum())} of {int(ref['days'].sum())}")
    return max(worst.values())


def _clips_both_ways(ref, A, what):
    """a case without clipping proves nothing: a clipped and a live scored day for each sign of A"""
    for sign in (1, -1):
        side = ref["m"] & (sign * A[:ref["m"].shape[0]] > 0)
        assert (side & ~ref["live"]).any() and (side & ref["live"]).any(), (what, sign)


def _sampled_schedule(C, ct, rb):
    """the alerts a sampled rollout issued from where the twins stand, with a policy that runs into the budget"""
    out = C.rollout(dict(_prefix_policy(ct), require_budget=rb, seed=19), alert_mask=True)
    st = C.state()
    assert bool((st["used"] >= st["budget"]).any())  # envs at the budget
    return out["alert_days"]


def _run(dev, data, what, pol_of, name="synth", n=N, prefix=9, n_steps=None, rb=False, sched_kind="hindsight",
         wkind="mixed", clip=CLIP, beta=0.0, grouped=True, kw=None, expect_clipping=True):
    """one case: old_log_prob from a perturbed copy of the policy, then the call under test against the stepped twin"""
    kw = kw or {}
    ct = data[name][0]
    A_, B = _make(dev, data, name, n, **kw), _make(dev, data, name, n, **kw)
    twins = [A_, B]
    if sched_kind == "sampled":
        twins.append(_make(dev, data, name, n, **kw))
    if prefix:
        for e_ in twins:
            _advance(e_, ct, prefix)
    g = _groups(n) if grouped else None
    pol = pol_of(ct, g)
    pol["require_budget"] = rb
    sched = _sampled_schedule(twins[2], ct, rb) if sched_kind == "sampled" else _schedule(sched_kind, A_, n, ct.T)
    w = _weights(n, wkind)
    S = ct.T if n_steps is None else n_steps
    adv = _advantage(S + 2, n)  # more call-days than the call runs: the rows past n_steps are not read
    old_pol = _perturbed_policy(pol)
    first = A_.surrogate_gradient(old_pol, sched, adv, clip=clip, entropy_coef=beta, env_weight=w, n_steps=n_steps, log_prob=True)
    lp0 = first["log_prob"]
    assert lp0.shape == (S, n) and lp0.dtype == torch.float32 and bool((lp0 <= 0).all())
    out = A_.surrogate_gradient(pol, sched, adv, old_log_prob=lp0, clip=clip, entropy_coef=beta, env_weight=w,
                                n_steps=n_steps, log_prob=True)
    assert A_.check_status() == 0
    R, _ = _step_reference(B, sched, S, rb)
    ng = G if grouped else 1
    A64, old64 = adv.astype(np.float64), lp0.double().cpu().numpy()
    ref0 = _restate(old_pol, R, w, A64, None, clip, beta, g, ng)
    r0 = _check(first, ref0, old_pol, what + " [epoch 0: rho = 1]")
    assert (first["clipped_days"] == 0).all() and (first["approx_kl"] == 0).all()
    ref = _restate(pol, R, w, A64, old64, clip, beta, g, ng)
    if pol["kind"] == "mlp":
        assert ref["near_kink"] < 0.01
    if expect_clipping:
        _clips_both_ways(ref, A64, what)
    r1 = _check(out, ref, pol, what)
    for e_ in twins:
        e_.close()
    return ref, out, max(r0, r1)


def _linear(ct, g, scale=0.4):
    W, b = _linear_params(ct, G if g is not None else 1, scale=scale)
    pol = dict(kind="linear", weight=W, bias=b, sample=True, seed=123)  # sample, seed: ignored
    if g is not None:
        pol["group"] = g
    return pol


def _mlp(net):
    def make(ct, g):
        _, hidden, act, n_out = MATRIX[net]
        k = G if g is not None else 1
        pol = dict(kind="mlp", layers=[(W[:k], b[:k]) for W, b in case_net(ct, net, hidden, n_out)], activation=act)
        if g is not None:
            pol["group"] = g
        return pol
    return make


ORDER = dict(lockstep=False, rollout_order=True)  # the handle's visiting order: not the identity
# name: keywords of _run
LINEAR = {
    "hindsight_order_rb": dict(rb=True, kw=ORDER, beta=0.01),
    "hindsight_n1": dict(n_steps=1, kw=ORDER),
    "hindsight_n3": dict(n_steps=3, beta=0.01),
    "sampled_at_budget_rb": dict(sched_kind="sampled", rb=True, beta=0.01),
    "sampled_at_budget": dict(sched_kind="sampled", rb=False),
    "clip0": dict(sched_kind="random", clip=0.0, beta=0.01, expect_clipping=False),
    "clip_large": dict(sched_kind="random", clip=1e6, rb=True, expect_clipping=False),
    "ragged_finished_on_entry": dict(name="ragged", prefix=25, sched_kind="random", beta=0.01),
    "slot27_one_group": dict(name="slot27", sched_kind="random", rb=True, wkind=None, grouped=False),
}


@pytest.mark.parametrize("case", list(LINEAR))
def test_linear_against_stepped_twin(dev, data, case):
    """300 envs, groups 0, 1, 3 of 4 (NaN rows for group 2), the handle's visiting order set; n_steps 1, 3 and the whole
    episode; envs finished on entry (ragged, a 25-day prefix); hindsight, random and sampled-at-the-budget schedules with
    require_budget on and off; weights with zeros and negative values; clip 0.2, 0 and one so large that nothing clips;
    entropy_coef 0 and 0.01; the ragged and slot-27 tables."""
    k = dict(LINEAR[case])
    # clip = 0 puts the edge at rho = 1, where every day on which both policies are saturated (lp = 0 to round-off) would
    # be ambiguous: that case takes a policy an eighth the size, whose logits stay far from saturation
    pol_of = (lambda ct, g: _linear(ct, g, scale=0.05)) if case == "clip0" else _linear
    ref, out, _ = _run(dev, data, "linear " + case, pol_of, **k)
    if case == "ragged_finished_on_entry":
        assert (~ref["m"][0]).any() and ref["m"][0].any()
    if case == "clip0":  # every scored day with A != 0 whose ratio is on the wrong side is clipped: about half of them
        assert 0.3 * ref["days"].sum() < ref["clipped"].sum()
    if case == "clip_large":
        assert (out["clipped_days"] == 0).all()
    if "rb" in case:
        assert (ref["days"] < ref["m"].shape[0]).any()


@pytest.mark.parametrize("net", list(MATRIX))
def test_mlp_every_instantiation_against_stepped_twin(dev, data, net):
    """The six <WIDTH, LAYERS> instantiations of k_sg_pass1 / k_pgm_pass2 with the nets of
    tests/policy_gradient_mlp_cases.py: 300 envs in the group-major order (not the identity), a 9-day prefix; schedule,
    require_budget, n_steps and entropy_coef alternate over the nets."""
    pair, hidden, act, n_out = MATRIX[net]
    i = list(MATRIX).index(net)
    _run(dev, data, f"<{pair[0]}, {pair[1]}> {net}", _mlp(net), rb=i % 2 == 1,
         sched_kind="random" if i % 5 == 4 else ("hindsight", "sampled", "random")[i % 3],
         n_steps=(None, None, 3, None, 1)[i % 5],  # one day: a random schedule (the hindsight one is nearly all zeros there)
         beta=(0.0, 0.01)[(i // 2) % 2])


@pytest.mark.parametrize("name", ["ragged", "slot27", "n8"])
def test_mlp_on_table_edges_and_the_n8_layout(dev, data, name):
    """<32, 2> on the ragged and slot-27 tables and <16, 2> on the 8-column observation layout, with an entropy bonus;
    the linear kind on the n8 layout as well."""
    if name == "n8":
        tb = L.make_table("n8")
        data = dict(data, n8=(tb.ct, dict(similar_climate_counties=True), L.RESET["n8"]["seed"], dict(L.RESET["n8"]["opts"])))
        _run(dev, data, "n8 linear", _linear, name="n8", prefix=5, sched_kind="random", rb=True, beta=0.01)
    net = "tanh7x13" if name == "n8" else "relu7x29_o2"
    _run(dev, data, f"{name} {net}", _mlp(net), name=name, prefix=5, sched_kind="random", rb=name != "ragged", beta=0.01)


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_without_old_log_prob_it_is_the_weighted_imitation_call(dev, data, kind):
    """old_log_prob=None, entropy_coef=0 agrees with imitation_gradient(day_weight=advantage) within the sum of the two
    restatements' bounds; "days" are equal; "log_prob" summed over the days agrees with "log_likelihood" within the sum
    of their bounds."""
    ct = data["synth"][0]
    A_, B = _make(dev, data, "synth", N), _make(dev, data, "synth", N)
    for e_ in (A_, B):
        _advance(e_, ct, 9)
    g = _groups(N)
    pol = dict((_linear if kind == "linear" else _mlp("tanh64x33_o2"))(ct, g), require_budget=True)
    sched = _schedule("random", A_, N, ct.T)
    w, adv = _weights(N, "mixed"), _advantage(ct.T, N)
    sg = A_.surrogate_gradient(pol, sched, adv, env_weight=w, log_prob=True)
    im = A_.imitation_gradient(pol, sched, env_weight=w, day_weight=torch.as_tensor(adv, device=dev))
    assert torch.equal(sg["days"], im["days"])
    R, _ = _step_reference(B, sched, ct.T, True)
    ref = _restate(pol, R, w, adv.astype(np.float64), None, CLIP, 0.0, g, G)
    args = (R["obs"], R["labels"], R["valid"], R["forced"], w)
    if kind == "linear":
        wi = weighted_imitation_linear_fp64(*args, adv, pol["weight"], pol["bias"], g, G)
        wi_parts = [wi["bound"]]
        ll = imitation_linear_fp64(*args, pol["weight"], pol["bias"], g, G)
    else:
        wi = weighted_imitation_mlp_fp64(*args, adv, pol["layers"], pol["activation"], g, G)
        wi_parts = [x for pair in wi["bound"] for x in pair]
        ll = imitation_mlp_fp64(*args, pol["layers"], pol["activation"], g, G)
    pgi = im["policy_gradient"]
    got_im = ([np.concatenate([pgi["weight"].double().cpu().numpy(), pgi["bias"].double().cpu().numpy()[:, None]], axis=1)]
              if kind == "linear" else [x.double().cpu().numpy() for pair in pgi["layers"] for x in pair])
    worst = 0.0
    for (got, want, bound), gi, bi in zip(_grad_parts(sg, ref, pol), got_im, wi_parts):
        have = ~np.isnan(want)
        diff = np.abs(got - gi)[have]
        worst = max(worst, _ratio(diff, (bound + bi)[have]))
        assert (diff <= (bound + bi)[have]).all(), (kind, worst)
    lsum = sg["log_prob"].double().sum(0).cpu().numpy()
    diff = np.abs(lsum - im["log_likelihood"].double().cpu().numpy())
    lb = ref["lp_bound"].sum(axis=0) + ll["ll_bound"]
    print(f"{kind}: max |surrogate - imitation(day_weight)| / (bound1 + bound2) = {worst:.3e}; "
          f"sum log_prob vs log_likelihood {_ratio(diff, lb):.3e}")
    assert (diff <= lb).all()
    A_.close()
    B.close()


def _flat(out):
    pg = out["policy_gradient"]
    parts = [pg["weight"], pg["bias"]] if "weight" in pg else [x for pair in pg["layers"] for x in pair]
    return parts + [out[k] for k in ("surrogate", "clipped_days", "approx_kl", "entropy", "days", "group_surrogate", "log_prob")]


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_no_side_effects_and_identical_bits(dev, data, kind):
    """Two identical calls return identical bits; state(), the observation buffer and a subsequent sampled rollout() are
    bit-identical to those of a twin that never made the call (mid-episode, after steps); the arguments are not written."""
    ct = data["synth"][0]
    A_, B = _make(dev, data, "synth", N), _make(dev, data, "synth", N)
    g = _groups(N)
    pol = dict((_linear if kind == "linear" else _mlp("relu7x29_o2"))(ct, g), require_budget=True)
    sched = _schedule("random", A_, N, ct.T)
    w = _weights(N, "mixed")
    adv = torch.as_tensor(_advantage(ct.T, N), device=dev)
    for e_ in (A_, B):
        for _ in range(3):
            e_.step(sched[:, 0].to(torch.int32))
    lp0 = A_.surrogate_gradient(_perturbed_policy(pol), sched, adv, env_weight=w, log_prob=True)["log_prob"]
    keep = (adv.clone(), lp0.clone())
    o1 = A_.surrogate_gradient(pol, sched, adv, old_log_prob=lp0, entropy_coef=0.01, env_weight=w, log_prob=True)
    o2 = A_.surrogate_gradient(pol, sched, adv, old_log_prob=lp0, entropy_coef=0.01, env_weight=w, log_prob=True)
    assert bool((o1["clipped_days"] > 0).any())
    for x, y in zip(_flat(o1), _flat(o2)):
        assert torch.equal(x.nan_to_num(7.0) if x.is_floating_point() else x, y.nan_to_num(7.0) if y.is_floating_point() else y)
    assert torch.equal(adv, keep[0]) and torch.equal(lp0, keep[1])
    sa, sb = A_.state(), B.state()
    for k in sb:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(A_._obs, B._obs) and A_.check_status() == 0
    roll = dict(_linear(ct, g), sample=True, seed=6)
    ra, rb_ = A_.rollout(roll, alert_mask=True), B.rollout(roll, alert_mask=True)
    assert set(ra) == set(rb_)
    for k, v in rb_.items():
        assert torch.equal(ra[k].nan_to_num(7.0) if v.is_floating_point() else ra[k], v.nan_to_num(7.0) if v.is_floating_point() else v), k
    assert torch.equal(A_._obs, B._obs)
    A_.close()
    B.close()


def test_refusals(dev, data):
    """A stale observation buffer (after load_state_dict) is a RuntimeError, as imitation_gradient()'s; bad arguments are
    ValueErrors before anything runs: the state is untouched."""
    ct = data["synth"][0]
    n = 65
    env = _make(dev, data, "synth", n)
    lin = _linear(ct, None)
    sched = _schedule("random", env, n, ct.T)
    adv = _advantage(ct.T, n)
    before = {k: v.clone() for k, v in env.state().items()}
    nan = adv.copy()
    nan[5, 3] = np.nan
    for pol, a, kw in (({"kind": "never"}, adv, {}), (lin, adv, dict(n_steps=0)), (lin, nan, {}), (lin, adv[:3], {}),
                       (lin, adv[:, :-1], {}), (lin, None, {}), (lin, adv, dict(old_log_prob=np.abs(adv))),
                       (lin, adv, dict(old_log_prob=-np.abs(adv[:3]))), (lin, adv, dict(clip=-0.1)),
                       (lin, adv, dict(clip=float("nan"))), (lin, adv, dict(entropy_coef=float("inf"))),
                       (lin, adv, dict(env_weight=np.full(n, np.nan))), (dict(lin, weight=lin["weight"][:, :-1]), adv, {})):
        with pytest.raises(ValueError):
            env.surrogate_gradient(pol, sched, a, **kw)
    with pytest.raises(ValueError):
        env.surrogate_gradient(lin, sched[:, :-1], adv)
    for k_, v in env.state().items():
        assert torch.equal(v, before[k_]), k_
    env.surrogate_gradient(lin, sched, adv[:3], n_steps=3)
    env.load_state_dict(env.state_dict())
    with pytest.raises(RuntimeError, match="observation buffer"):
        env.surrogate_gradient(lin, sched, adv)
    env.close()
    fx = _make(dev, data, "synth", n, fixes=["lag"])
    with pytest.raises(ValueError):
        fx.surrogate_gradient(lin, sched, adv)
    fx.close()
