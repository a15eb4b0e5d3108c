"""What the learned-policy entry points refuse before they look at the handle, and in which order.

Every exported entry point between w2a_rollout_linear and w2a_value_gradient_mlp_gae that takes a handle (24: the plain,
_record, _gated and _weighted forms and the value and GAE calls) is called with a NULL handle and a table of arguments
of which one is bad: the call returns W2A_ERR_ARG and w2a_last_error() is the entry point's name and that check's text,
in full. With two bad arguments the check that comes first in the body is the one reported, which pins the order of the
checks; with none the call ends at "NULL handle". Nothing is launched (there is no device here), and the fake pointers
are never read: the handle is checked before anything dereferences them. The eight workspace-size queries of the same
region take no handle; their values are pinned against the layouts include/w2a.h documents."""
import ctypes as C
import itertools

import pytest

from weather2alert_amd import _ffi, build

P = 4096  # a non-NULL, 256-B aligned address that is never read
NAN, INF = float("nan"), float("inf")
OBS = "NULL obs (the rows the agent holds are the first day's input)"
WS = [({"workspace": None}, "NULL workspace"), ({"workspace": P + 64}, "workspace must be 256-B aligned")]
GATE = ("allowed_days", "allowed_words")


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


# ---- the checks of each family, in the order of the body: ([mutations with one text], text) ---------------------------
def linear_struct(who, sample):
    """sample: "01" (0 or 1), "1" (must be 1) or None (sample and require_budget are ignored: the value calls)"""
    c = [({"policy": None}, f"NULL {who}"), ({"n_steps": 0}, "n_steps must be positive"),
         ({"p.weight": None}, "NULL weight or bias"), ({"p.bias": None}, "NULL weight or bias"),
         ({"p.n_groups": 0}, "n_groups must be positive")]
    c += sample_rule(sample)
    return c + [({"p.weight": P + 4}, "weight must be 16-B aligned")]


def mlp_struct(who, sample):
    c = [({"policy": None}, f"NULL {who}"), ({"n_steps": 0}, "n_steps must be positive"),
         ({"p.params": None}, "NULL params"), ({"p.n_groups": -1}, "n_groups must be positive"),
         ({"p.n_layers": 3}, "n_layers must be 1 or 2"), ({"p.width": 48}, "width must be 16, 32 or 64"),
         ({"p.activation": 2}, "activation must be W2A_MLP_TANH or W2A_MLP_RELU")]
    c += sample_rule(sample)
    return c + [({"p.params": P + 16 + 8}, "params must be 16-B aligned")]


def sample_rule(sample):
    if sample is None:
        return []
    first = (({"p.sample": 2}, "sample must be 0 or 1") if sample == "01" else
             ({"p.sample": 0}, "sample must be 1 (a deterministic policy has no score function)"))
    return [first, ({"p.require_budget": 2}, "require_budget must be 0 or 1")]


def struct(kind, who, sample):
    return linear_struct(who, sample) if kind == "linear" else mlp_struct(who, sample)


TRAJ = [({"t." + k: None}, "NULL trajectory array") for k in ("obs", "logit", "reward", "action", "flags")]
ROLLOUT = ("n_steps", "obs", "ret_out", "alerts_out", "attempts_over_budget", "alert_mask", "attempt_mask", "mask_words",
           "last_return", "ret_snapshot", "stream")
ROLLOUT_OK = dict(n_steps=3, obs=P, ret_out=P, alerts_out=None, attempts_over_budget=None, alert_mask=P, attempt_mask=None,
                  mask_words=0, last_return=None, ret_snapshot=None, stream=None)


def rollout(kind, form):
    names, checks = ROLLOUT, struct(kind, "policy", "01") + [({"obs": None}, OBS)]
    if form == "_record":  # the trajectory is required and checked before the policy
        names, checks = names + ("traj",), [({"traj": None}, "NULL trajectory")] + TRAJ + checks
    if form == "_gated":  # ... here it may be NULL
        names, checks = names + ("traj",) + GATE, TRAJ + checks
    return names, dict(ROLLOUT_OK), checks, []


def policy_gradient(kind, form):
    names = ("baseline", "n_steps", "obs", "grad", "workspace", "workspace_bytes", "stream") + (GATE if form else ())
    ok = dict(baseline=1, n_steps=3, obs=P, grad=P, workspace=P, workspace_bytes=1 << 20, stream=None)
    checks = struct(kind, "policy", "1") + [
        ({"baseline": 2}, "baseline must be W2A_PG_BASELINE_NONE or W2A_PG_BASELINE_NO_ALERT"), ({"obs": None}, OBS),
        ({"grad": None}, "NULL grad or workspace"), ({"workspace": None}, "NULL grad or workspace"), WS[1]]
    return names, ok, checks, []


def imitation(kind, form):
    weighted = ("day_weight", "day_weight_days") if form else ()
    names = (("alert_mask", "mask_words", "env_weight") + weighted + ("n_steps", "obs", "grad", "loglik", "days") +
             (("workspace", "workspace_bytes") if kind == "mlp" else ()) + ("stream",) + (GATE if form == "_gated" else ()))
    ok = dict(alert_mask=P, mask_words=0, env_weight=None, day_weight=P, day_weight_days=3, n_steps=3, obs=P, grad=P,
              loglik=P, days=P, workspace=P, workspace_bytes=1 << 20, stream=None)
    checks = struct(kind, "policy", "01") + [({"alert_mask": None}, "NULL alert_mask (the schedule to score)"), ({"obs": None}, OBS)]
    checks += [({k: None}, "NULL grad, loglik or days") for k in ("grad", "loglik", "days")]
    if kind == "mlp":
        checks += WS
    if form:
        checks += [({"day_weight_days": 2}, "day_weight holds fewer call-days than n_steps")]
    # a NULL day_weight weighs every day 1, whatever its count says
    return names, ok, checks, ([({"day_weight": None, "day_weight_days": 0}, "NULL handle")] if form else [])


def surrogate(kind, form):
    names = (("alert_mask", "mask_words", "env_weight", "advantage", "advantage_days", "old_log_prob", "old_log_prob_days",
              "clip", "entropy_coef", "n_steps", "obs", "grad", "surrogate", "clipped_days", "approx_kl", "entropy", "days",
              "log_prob") + (("workspace", "workspace_bytes") if kind == "mlp" else ()) + ("stream",) + (GATE if form else ()))
    ok = dict(alert_mask=P, mask_words=0, env_weight=None, advantage=P, advantage_days=3, old_log_prob=P,
              old_log_prob_days=3, clip=0.2, entropy_coef=0.01, n_steps=3, obs=P, grad=P, surrogate=P, clipped_days=P,
              approx_kl=P, entropy=P, days=P, log_prob=None, workspace=P, workspace_bytes=1 << 20, stream=None)
    checks = struct(kind, "policy", "01") + [({"alert_mask": None}, "NULL alert_mask (the schedule to score)"), ({"obs": None}, OBS)]
    checks += [({k: None}, "NULL grad, surrogate, clipped_days, approx_kl, entropy or days")
               for k in ("grad", "surrogate", "clipped_days", "approx_kl", "entropy", "days")]
    if kind == "mlp":  # the workspace sits between the outputs and the inputs
        checks += WS
    checks += [({"advantage": None}, "NULL advantage"), ({"advantage_days": 2}, "advantage holds fewer call-days than n_steps"),
               ({"old_log_prob_days": 2}, "old_log_prob holds fewer call-days than n_steps")]
    checks += [({"clip": v}, "clip must be finite and not negative") for v in (-0.1, NAN, INF)]
    checks += [({"entropy_coef": v}, "entropy_coef must be finite") for v in (NAN, -INF)]
    # without old_log_prob the first epoch's ratio is 1, whatever its count says
    return names, ok, checks, [({"old_log_prob": None, "old_log_prob_days": 0}, "NULL handle")]


def value(kind, form):
    gae = ("gamma", "lambda", "bootstrap", "value_target", "target", "target_days") if form else ()
    names = (("alert_mask", "mask_words", "env_weight", "n_steps", "obs", "grad", "sq_error", "days", "ret", "advantage") + gae +
             ("workspace", "workspace_bytes", "stream"))
    ok = dict(alert_mask=P, mask_words=0, env_weight=None, n_steps=3, obs=P, grad=P, sq_error=P, days=P, ret=P,
              advantage=None, gamma=1.0, bootstrap=0, value_target=None, target=None, target_days=0, workspace=P,
              workspace_bytes=1 << 20, stream=None)
    ok["lambda"] = 1.0
    checks = struct(kind, "value", None) + [({"alert_mask": None}, "NULL alert_mask (the schedule to follow)"), ({"obs": None}, OBS)]
    checks += [({k: None}, "NULL grad, sq_error, days or ret") for k in ("grad", "sq_error", "days", "ret")]
    extra = [({"p.sample": 7, "p.require_budget": 7}, "NULL handle")]  # a value network has neither
    if form:  # the GAE checks sit between the outputs and the workspace
        given = {"target": P, "target_days": 3}
        formed = "advantage and value_target are not formed when target is given"
        meaning = "gamma, lambda and bootstrap have no meaning when target is given"
        checks += [({"gamma": v}, "gamma must lie in [0, 1]") for v in (1.5, -0.5, NAN)]
        checks += [({"lambda": v}, "lambda must lie in [0, 1]") for v in (1.5, -0.5, NAN)]
        checks += [({"bootstrap": 2}, "bootstrap must be 0 or 1"),
                   ({"target": P, "target_days": 2}, "target holds fewer call-days than n_steps"),
                   ({**given, "advantage": P}, formed), ({**given, "value_target": P}, formed),
                   ({**given, "gamma": 0.5}, meaning), ({**given, "lambda": 0.5}, meaning), ({**given, "bootstrap": 1}, meaning)]
        extra += [({**given, "target_days": 2, "advantage": P, "gamma": 0.5}, "target holds fewer call-days than n_steps"),
                  ({**given, "value_target": P, "bootstrap": 1}, formed), (given, "NULL handle"),
                  ({"advantage": P, "value_target": P, "gamma": 0.9, "lambda": 0.0, "bootstrap": 1}, "NULL handle")]
    return names, ok, checks + WS, extra


ENTRY_POINTS = (
    [("w2a_rollout_" + k + f, rollout, k, f) for k in ("linear", "mlp") for f in ("", "_record", "_gated")] +
    [("w2a_policy_gradient_" + k + f, policy_gradient, k, f) for k in ("linear", "mlp") for f in ("", "_gated")] +
    [("w2a_imitation_gradient_" + k + f, imitation, k, f) for k in ("linear", "mlp") for f in ("", "_weighted", "_gated")] +
    [("w2a_surrogate_gradient_" + k + f, surrogate, k, f) for k in ("linear", "mlp") for f in ("", "_gated")] +
    [("w2a_value_gradient_" + k + f, value, k, f) for k in ("linear", "mlp") for f in ("", "_gae")])


def _call(lib, name, kind, names, ok, bad):
    """one call with a NULL handle: `ok` with the entries of `bad` put in ("p.x": a field of the policy struct, "t.x":
    of the trajectory, "policy" / "traj": the struct's pointer itself); returns (return code, error text)"""
    if kind == "linear":
        pol = _ffi.LinearPolicy(weight=P, bias=P, group=None, n_groups=1, sample=1, require_budget=0, seed=0)
    else:
        pol = _ffi.MlpPolicy(params=P, group=None, order=None, n_groups=1, n_layers=2, width=64, activation=0, sample=1,
                             require_budget=0, seed=0)
    traj = _ffi.Trajectory(obs=P, logit=P, reward=P, action=P, flags=P)
    a = dict(ok, policy=C.byref(pol), traj=C.byref(traj), allowed_days=P, allowed_words=0)
    for k, v in bad.items():
        if k.startswith("p."):
            setattr(pol, k[2:], v)
        elif k.startswith("t."):
            setattr(traj, k[2:], v)
        else:
            a[k] = v
    rc = getattr(lib, name)(None, a["policy"], *(a[k] for k in names))
    return rc, lib.w2a_last_error().decode()


def test_the_24_entry_points_are_all_of_the_region():
    listed = {e[0] for e in ENTRY_POINTS}
    region = {s for s in _ffi.SYMBOLS if s.startswith(("w2a_rollout_linear", "w2a_rollout_mlp", "w2a_policy_gradient_",
                                                        "w2a_imitation_gradient_", "w2a_surrogate_gradient_",
                                                        "w2a_value_gradient_")) and not s.endswith("_workspace_bytes")}
    assert len(ENTRY_POINTS) == len(listed) == 24 and listed == region


@pytest.mark.parametrize("name,family,kind,form", ENTRY_POINTS, ids=[e[0] for e in ENTRY_POINTS])
def test_refusals_and_their_order(lib, name, family, kind, form):
    names, ok, checks, extra = family(kind, form)
    assert len(names) + 2 == len(getattr(lib, name).argtypes)
    assert _call(lib, name, kind, names, ok, {}) == (-1, f"{name}: NULL handle")
    if "allowed_days" in names:  # the gate is looked at after the handle; a NULL trajectory records nothing
        assert _call(lib, name, kind, names, ok, {"allowed_days": None}) == (-1, f"{name}: NULL handle")
        if "traj" in names:
            assert _call(lib, name, kind, names, ok, {"traj": None}) == (-1, f"{name}: NULL handle")
    for bad, text in checks + extra:
        assert _call(lib, name, kind, names, ok, bad) == (-1, f"{name}: {text}"), bad
    # two bad arguments: the earlier check reports (pairs that set one argument twice say nothing)
    pairs = 0
    for (bad1, text1), (bad2, _) in itertools.combinations(checks, 2):
        if bad1.keys() & bad2.keys():
            continue
        assert _call(lib, name, kind, names, ok, {**bad2, **bad1}) == (-1, f"{name}: {text1}"), (bad1, bad2)
        pairs += 1
    assert pairs > len(checks)


def _align256(x):
    return (x + 255) // 256 * 256


def test_workspace_sizes(lib):
    """the eight size queries of the region: 8 + 1 B per env-day for the linear gradient calls, 8 + 8 + 1 B for linear
    GAE, each array on its own 256-B boundary; the five MLP queries are one layout; nothing for shapes no call accepts"""
    for n, s in ((1000, 153), (70_001, 7), (1, 1)):
        days = n * s
        assert lib.w2a_policy_gradient_workspace_bytes(n, s) == _align256(8 * days) + _align256(days)
        assert lib.w2a_value_gradient_linear_workspace_bytes(n, s) == _align256(8 * days) + _align256(days)
        assert lib.w2a_value_gradient_linear_gae_workspace_bytes(n, s) == 2 * _align256(8 * days) + _align256(days)
    for f in ("w2a_policy_gradient_workspace_bytes", "w2a_value_gradient_linear_workspace_bytes",
              "w2a_value_gradient_linear_gae_workspace_bytes"):
        assert getattr(lib, f)(0, 10) == 0 and getattr(lib, f)(100, 0) == 0 and getattr(lib, f)(-1, 10) == 0
    mlp = [getattr(lib, f"w2a_{f}_workspace_bytes") for f in ("policy_gradient_mlp", "imitation_gradient_mlp",
                                                               "surrogate_gradient_mlp", "value_gradient_mlp",
                                                               "value_gradient_mlp_gae")]
    for size in mlp:
        for shape in ((100, 10, 1, 16, 1), (70_000, 153, 5, 64, 2), (1, 1, 3, 32, 2)):
            n, s, g, w, layers = shape
            assert size(*shape) == mlp[0](*shape) and size(*shape) % 256 == 0
            # pass 1's scratch (9 B per env-day, 12 B per env) and at least one fp64 partial block per wave of pass 2
            stride = 32 * w + w + (w * w + w if layers == 2 else 0) + w + 4  # W2A_MLP_STRIDE
            assert size(*shape) >= 9 * n * s + 12 * n + 8 * stride
        for shape in ((0, 10, 1, 16, 1), (100, 0, 1, 16, 1), (100, 10, 0, 16, 1), (100, 10, 1, 48, 1), (100, 10, 1, 16, 3)):
            assert size(*shape) == 0
