"""fisher_vector_product() (k_fisher_linear; k_fv_pass1 + the second pass of w2a_policy_gradient_mlp) against the fp64
restatement (tests/fisher_restatement.py). The reference never touches the kernels under test: an identical twin from
the same seed is stepped day by day through step() with the schedule's actions (tests/test_imitation_gpu.py's
_step_reference) and the rows it returns go to the restatement. Every comparison requires |got - ref| <= bound for every
component of the product, of "quadratic" and of "group_quadratic", equal "days", NaN exactly where the reference has an
empty group and at most AMBIGUOUS_CAP of the ReLU unit-days near a kink, and prints the largest ratio to the bound.
Shapes: 300 envs (four full waves and a partial one), groups 0, 1, 3 of 4 interleaved (group boundaries inside waves for
the linear kind; the MLP kind visits group-major, so its waves hold two groups where one group ends), group 2 empty."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fisher_restatement import AMBIGUOUS_CAP, fisher_linear_fp64, fisher_mlp_fp64  # noqa: E402
from imitation_restatement import attempts_from_schedule  # noqa: E402
from policy_gradient_mlp_cases import MATRIX  # noqa: E402
from test_imitation_gpu import (_advance, _make, _ratio, _schedule, _step_reference, _weights, data, dev)  # noqa: E402,F401
from test_surrogate_gpu import ORDER, _groups, _linear, _mlp, _sampled_schedule  # noqa: E402

pytestmark = pytest.mark.gpu

N, G = 300, 4


def _vector(pol, seed=41):
    """a random vector in the shape of the policy's "policy_gradient" (f32: what the kernels read)"""
    rng = np.random.default_rng(seed)
    if pol["kind"] == "linear":
        return {"weight": rng.standard_normal(pol["weight"].shape).astype(np.float32),
                "bias": rng.standard_normal(pol["bias"].shape).astype(np.float32)}
    return {"layers": [(rng.standard_normal(np.shape(W)).astype(np.float32) / np.float32(np.sqrt(np.shape(W)[-1])),
                        rng.standard_normal(np.shape(b)).astype(np.float32)) for W, b in pol["layers"]]}


def _restate(pol, vec, R, forced, w, g, n_groups):
    args = (R["obs"], R["labels"], R["valid"], forced, w)
    if pol["kind"] == "linear":
        return fisher_linear_fp64(*args, pol["weight"], pol["bias"], vec["weight"], vec["bias"], g, n_groups)
    return fisher_mlp_fp64(*args, pol["layers"], vec["layers"], pol["activation"], g, n_groups)


def _parts(fv, ref, pol):
    """[(got, want, bound), ...] over the parameter arrays"""
    if pol["kind"] == "linear":
        got = np.concatenate([fv["weight"].double().cpu().numpy(), fv["bias"].double().cpu().numpy()[:, None]], axis=1)
        return [(got, np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1), ref["bound"])]
    G_ = ref["layers"][0][0].shape[0]
    assert [(tuple(a.shape), tuple(b.shape)) for a, b in fv["layers"]] == \
        [((G_,) + np.shape(W)[-2:], (G_,) + np.shape(b)[-1:]) for W, b in pol["layers"]]
    parts = []
    for (dW, db), (rW, rb), (bW, bb) in zip(fv["layers"], ref["layers"], ref["bound"]):
        parts += [(dW.double().cpu().numpy(), rW, bW), (db.double().cpu().numpy(), rb, bb)]
    return parts


def _check(out, ref, pol, what):
    """every component within its bound; returns the largest ratio to the bound"""
    assert ref["near_kink"] <= AMBIGUOUS_CAP, (what, ref["near_kink"])
    worst = {"product": 0.0}
    for got, want, bound in _parts(out["fisher_vector_product"], ref, pol):
        empty = np.isnan(want)
        assert np.isnan(got[empty]).all() and np.isfinite(got[~empty]).all(), what  # NaN for a group without envs
        diff = np.abs(got - want)[~empty]
        worst["product"] = max(worst["product"], _ratio(diff, bound[~empty]))
        assert (diff <= bound[~empty]).all(), (what, "product", worst)
    assert out["quadratic"].dtype == torch.float32 and out["days"].dtype == torch.int32
    diff = np.abs(out["quadratic"].double().cpu().numpy() - ref["quadratic"])
    worst["quadratic"] = _ratio(diff, ref["quadratic_bound"])
    assert (diff <= ref["quadratic_bound"]).all(), (what, "quadratic", worst)
    np.testing.assert_array_equal(out["days"].cpu().numpy(), ref["days"], err_msg=what)
    gq = out["group_quadratic"].double().cpu().numpy()
    have = ~np.isnan(ref["group_quadratic"])
    assert gq.shape == have.shape and np.isnan(gq[~have]).all() and np.isfinite(gq[have]).all(), what
    diff = np.abs(gq - ref["group_quadratic"])[have]
    worst["group_quadratic"] = _ratio(diff, ref["group_quadratic_bound"][have])
    assert (diff <= ref["group_quadratic_bound"][have]).all(), (what, "group_quadratic", worst)
    assert np.abs(ref["quadratic"]).max() > 0, what  # a case that scores nothing proves nothing
    print(f"{what}: ratio to the bound " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items())
          + f"; near-kink share {ref['near_kink']:.2e}, scored days {int(ref['days'].sum())}")
    return max(worst.values())


def _run(dev, data, what, pol_of, name="synth", n=N, prefix=9, n_steps=None, rb=False, sched_kind="hindsight",
         wkind="mixed", grouped=True, kw=None, gate=None):
    """one case: the call under test against the stepped twin"""
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
    vec = _vector(pol)
    call, followed = dict(pol), sched
    t0 = A_.state()["t"].cpu().numpy()
    if gate is not None:
        allowed = A_.alert_gate("heat_qi", gate)
        assert allowed.dtype == torch.bool and tuple(allowed.shape) == (n, ct.T)
        call["allowed_days"] = allowed
        followed = sched & allowed  # the twin attempts what the gate lets through
    out = A_.fisher_vector_product(call, sched, vec, env_weight=w, n_steps=n_steps)
    sg = A_.surrogate_gradient(call, sched, np.zeros((S, n), np.float32), env_weight=w, n_steps=n_steps)
    assert torch.equal(out["days"], sg["days"])
    assert A_.check_status() == 0
    R, _ = _step_reference(B, followed, S, rb)
    forced = R["forced"]
    if gate is not None:
        closed = ~attempts_from_schedule(allowed.cpu().numpy(), t0, R["valid"]) & R["valid"]
        assert (closed & ~forced).any() and (R["valid"] & ~closed & ~forced).any()  # closed and open days while budget is left
        forced = forced | closed
    ref = _restate(pol, vec, R, forced, w, g, G if grouped else 1)
    r = _check(out, ref, pol, what)
    for e_ in twins:
        e_.close()
    return ref, out, R, forced, r


# name: keywords of _run
LINEAR = {
    "hindsight_order_rb": dict(rb=True, kw=ORDER),
    "hindsight": dict(rb=False),
    "sampled_at_budget_rb": dict(sched_kind="sampled", rb=True),
    "sampled_at_budget": dict(sched_kind="sampled", rb=False),
    "chunk_n3": dict(n_steps=3, sched_kind="random"),
    "chunk_n1": dict(n_steps=1, sched_kind="random", kw=ORDER),
    "no_prefix": dict(prefix=0, sched_kind="random", rb=True),
    "gate_rb": dict(sched_kind="random", rb=True, gate=0.6),
    "gate": dict(sched_kind="random", rb=False, gate=0.6),
    "ragged_finished_on_entry": dict(name="ragged", prefix=25, sched_kind="random"),
    "slot27_one_group": dict(name="slot27", sched_kind="random", rb=True, wkind=None, grouped=False),
}


@pytest.mark.parametrize("case", list(LINEAR))
def test_linear_against_stepped_twin(dev, data, case):
    """300 envs, groups 0, 1, 3 of 4 (NaN rows for group 2), the handle's visiting order set and unset; a 9-day prefix
    and none; n_steps 1, 3 and the whole episode; envs finished on entry (ragged, a 25-day prefix); hindsight, random and
    sampled-at-the-budget schedules with require_budget on and off; "allowed_days" from alert_gate(); weights with zeros,
    negative values and mixed magnitudes, and none; one group with group=None; the ragged and slot-27 tables."""
    ref, out, R, forced, _ = _run(dev, data, "linear " + case, _linear, **LINEAR[case])
    if case == "ragged_finished_on_entry":
        assert (~R["valid"][0]).any() and R["valid"][0].any()
        fin = ~R["valid"][0]
        assert (out["quadratic"].cpu().numpy()[fin] == 0).all() and (out["days"].cpu().numpy()[fin] == 0).all()
    if "rb" in case:
        assert (ref["days"] < R["valid"].sum(axis=0)).any()  # days that require_budget (or the gate) took out
    if case == "slot27_one_group":
        assert out["group_quadratic"].shape == (1,)


@pytest.mark.parametrize("net", list(MATRIX))
def test_mlp_every_instantiation_against_stepped_twin(dev, data, net):
    """The six <WIDTH, LAYERS> instantiations of k_fv_pass1 / mlp_logit_jvp with the nets of
    tests/policy_gradient_mlp_cases.py (padded units, tanh and ReLU, one- and two-row outputs): 300 envs in the
    group-major order, a 9-day prefix; schedule, require_budget, n_steps and the gate alternate over the nets."""
    pair, hidden, act, n_out = MATRIX[net]
    i = list(MATRIX).index(net)
    _run(dev, data, f"<{pair[0]}, {pair[1]}> {net}", _mlp(net), rb=i % 2 == 1,
         sched_kind=("hindsight", "sampled", "random")[i % 3], n_steps=(None, None, 3, None, None)[i % 5],
         gate=0.6 if i % 4 == 2 else None)


@pytest.mark.parametrize("name", ["ragged", "slot27"])
def test_mlp_on_table_edges(dev, data, name):
    """<32, 2> ReLU with a two-row output on the ragged tables (envs finished on entry) and on the slot-27 tables with
    one group and no weights"""
    if name == "ragged":
        _, out, R, _, _ = _run(dev, data, "ragged relu7x29_o2", _mlp("relu7x29_o2"), name=name, prefix=25, sched_kind="random")
        fin = ~R["valid"][0]
        assert fin.any() and (out["quadratic"].cpu().numpy()[fin] == 0).all()
    else:
        _run(dev, data, "slot27 relu7x29_o2", _mlp("relu7x29_o2"), name=name, prefix=5, sched_kind="random", rb=True,
             wkind=None, grouped=False)


def _flat(fv):
    return [fv["weight"], fv["bias"]] if "weight" in fv else [x for pair in fv["layers"] for x in pair]


def _inner(vec, fv):
    """<vec, fv> per group, in fp64"""
    va = [vec["weight"], vec["bias"]] if "weight" in vec else [x for pair in vec["layers"] for x in pair]
    dot = sum((np.asarray(v, np.float64) * f.double().cpu().numpy()).reshape(f.shape[0], -1).sum(axis=1)
              for v, f in zip(va, _flat(fv)))
    return dot


def _inner_bound(vec, ref, pol):
    va = [vec["weight"], vec["bias"]] if "weight" in vec else [x for pair in vec["layers"] for x in pair]
    if pol["kind"] == "linear":
        v1 = np.concatenate([np.abs(va[0]), np.abs(va[1])[:, None]], axis=1).astype(np.float64)
        return (v1 * ref["bound"]).sum(axis=1)
    bs = [x for pair in ref["bound"] for x in pair]
    return sum((np.abs(np.asarray(v, np.float64)) * b).reshape(b.shape[0], -1).sum(axis=1) for v, b in zip(va, bs))


@pytest.mark.parametrize("kind", ["linear", "tanh29x9", "relu40x64"])
def test_properties_of_the_product(dev, data, kind):
    """On the shapes above, mid-episode, with require_budget: <v, F_g v> formed on the host from the returned product
    equals group_quadratic[g] within the sum of their bounds; <u, F v> = <v, F u> for two random vectors within the
    bounds; group_quadratic >= 0 for env_weight >= 0; vector = 0 gives exact zeros; two identical calls give identical
    bits; state, observation buffer and status word are bit-identical before and after; the arguments are not written.
    (One-row outputs: a two-row vector's fold is rounded to f32 on the way in, which <u, F v> on the unfolded rows
    would see.)"""
    ct = data["synth"][0]
    A_, B = _make(dev, data, "synth", N), _make(dev, data, "synth", N)
    for e_ in (A_, B):
        _advance(e_, ct, 9)
    g = _groups(N)
    pol = dict((_linear if kind == "linear" else _mlp(kind))(ct, g), require_budget=True)
    sched = _schedule("random", A_, N, ct.T)
    w = np.abs(_weights(N, "mixed"))
    v, u = _vector(pol, 41), _vector(pol, 43)
    before = {k: x.clone() for k, x in A_.state().items()}
    obs0, status0 = A_._obs.clone(), A_.status_word.clone()
    keep = [np.array(x, copy=True) for x in ([v["weight"], v["bias"]] if kind == "linear" else [y for p in v["layers"] for y in p])]
    Fv = A_.fisher_vector_product(pol, sched, v, env_weight=w)
    Fv2 = A_.fisher_vector_product(pol, sched, v, env_weight=w)
    Fu = A_.fisher_vector_product(pol, sched, u, env_weight=w)
    after = A_.state()
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert torch.equal(obs0, A_._obs) and torch.equal(status0, A_.status_word) and A_.check_status() == 0
    for x, y in zip(keep, ([v["weight"], v["bias"]] if kind == "linear" else [y for p in v["layers"] for y in p])):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(_flat(Fv["fisher_vector_product"]) + [Fv[k] for k in ("quadratic", "days", "group_quadratic")],
                    _flat(Fv2["fisher_vector_product"]) + [Fv2[k] for k in ("quadratic", "days", "group_quadratic")]):
        assert torch.equal(x.nan_to_num(7.0) if x.is_floating_point() else x, y.nan_to_num(7.0) if y.is_floating_point() else y)
    R, _ = _step_reference(B, sched, ct.T, True)
    ref_v, ref_u = _restate(pol, v, R, R["forced"], w, g, G), _restate(pol, u, R, R["forced"], w, g, G)
    have = ~np.isnan(ref_v["group_quadratic"])
    gq = Fv["group_quadratic"].double().cpu().numpy()
    assert (gq[have] >= 0).all() and (Fv["quadratic"] >= 0).all()
    vFv = _inner(v, Fv["fisher_vector_product"])
    tol = _inner_bound(v, ref_v, pol) + ref_v["group_quadratic_bound"]
    r1 = _ratio(np.abs(vFv - gq)[have], tol[have])
    assert (np.abs(vFv - gq)[have] <= tol[have]).all(), (kind, r1)
    uFv, vFu = _inner(u, Fv["fisher_vector_product"]), _inner(v, Fu["fisher_vector_product"])
    tol = _inner_bound(u, ref_v, pol) + _inner_bound(v, ref_u, pol)
    r2 = _ratio(np.abs(uFv - vFu)[have], tol[have])
    assert (np.abs(uFv - vFu)[have] <= tol[have]).all(), (kind, r2)
    # the symmetry is not one of two zeros, nor the bound a blanket: the terms of the inner product outweigh it
    mag = _inner({k_: ([(np.abs(W), np.abs(b)) for W, b in x] if k_ == "layers" else np.abs(x)) for k_, x in u.items()},
                 {k_: ([(W.abs(), b.abs()) for W, b in x] if k_ == "layers" else x.abs()) for k_, x in Fv["fisher_vector_product"].items()})
    assert (mag[have] > tol[have]).all() and (np.abs(uFv)[have] > 0).all(), (mag, tol)
    print(f"{kind}: |<v, Fv> - group_quadratic| / bound = {r1:.3e}; |<u, Fv> - <v, Fu>| / bound = {r2:.3e}; "
          f"bound / sum of |u_i (Fv)_i| = {float((tol / mag)[have].max()):.3e}")
    zero = ({"weight": np.zeros_like(v["weight"]), "bias": np.zeros_like(v["bias"])} if kind == "linear" else
            {"layers": [(np.zeros_like(W), np.zeros_like(b)) for W, b in v["layers"]]})
    F0 = A_.fisher_vector_product(pol, sched, zero, env_weight=w)
    for x in _flat(F0["fisher_vector_product"]):
        assert bool((x[torch.as_tensor(have)] == 0).all()) and bool(torch.isnan(x[torch.as_tensor(~have)]).all())
    assert bool((F0["quadratic"] == 0).all()) and torch.equal(F0["days"], Fv["days"])
    assert bool((F0["group_quadratic"][torch.as_tensor(have)] == 0).all())
    # the logit is mlp_logit's, bit for bit: p_s agrees with every other call on the same episodes
    lp = A_.surrogate_gradient(pol, sched, np.zeros((ct.T, N), np.float32), env_weight=w, log_prob=True)
    assert torch.equal(lp["days"], Fv["days"])
    A_.close()
    B.close()


def test_refusals(dev, data):
    """A stale observation buffer (after load_state_dict) is a RuntimeError, as surrogate_gradient()'s; bad arguments are
    ValueErrors before anything runs: the state is untouched."""
    ct = data["synth"][0]
    n = 65
    env = _make(dev, data, "synth", n)
    lin = _linear(ct, None)
    sched = _schedule("random", env, n, ct.T)
    v = _vector(lin)
    before = {k: x.clone() for k, x in env.state().items()}
    nan = dict(v, weight=v["weight"].copy())
    nan["weight"][0, 2] = np.nan
    for pol, vec, kw in (({"kind": "never"}, v, {}), (lin, v, dict(n_steps=0)), (lin, nan, {}), (lin, None, {}),
                         (lin, dict(v, weight=v["weight"][:, :-1]), {}), (lin, {"layers": []}, {}),
                         (lin, dict(v, bias=np.zeros(2, np.float32)), {}), (lin, v, dict(env_weight=np.full(n, np.nan))),
                         (dict(lin, weight=lin["weight"][:, :-1]), v, {})):
        with pytest.raises(ValueError):
            env.fisher_vector_product(pol, sched, vec, **kw)
    with pytest.raises(ValueError):
        env.fisher_vector_product(lin, sched[:, :-1], v)
    for k_, x in env.state().items():
        assert torch.equal(x, before[k_]), k_
    env.fisher_vector_product(lin, sched, v, n_steps=3)
    env.load_state_dict(env.state_dict())
    with pytest.raises(RuntimeError, match="observation buffer"):
        env.fisher_vector_product(lin, sched, v)
    env.close()
    fx = _make(dev, data, "synth", n, fixes=["lag"])
    with pytest.raises(ValueError):
        fx.fisher_vector_product(lin, sched, v)
    fx.close()
