"""policy["lookahead"] on the host: the checks of weather2alert_amd/policy.py, the refusals of the env's entry points
(every one is raised before anything touches a device), the packing of the MLP tail and its adjoint, the header's
constants, and the restatement alone (tests/lookahead_restatement.py) on the mini and ragged tables."""
import os
import re

import numpy as np
import pytest
import torch

import lookahead_cases as C
import lookahead_restatement as LR
import policy_gradient_mlp_cases as M
import table_edges as E
from weather2alert_amd import HeatAlertVecEnv, _ffi, policy as P, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = open(os.path.join(ROOT, "include", "w2a.h")).read()
NEW_SYMBOLS = ("w2a_lookahead_rollout_linear", "w2a_lookahead_rollout_linear_gated", "w2a_lookahead_rollout_mlp",
               "w2a_lookahead_rollout_mlp_gated", "w2a_lookahead_policy_gradient_linear",
               "w2a_lookahead_imitation_gradient_linear")


@pytest.fixture(scope="module")
def ct():
    return tables.CompiledTables.load_npz(os.path.join(GOLDEN, "mini_compiled.npz"))


@pytest.fixture(scope="module")
def ragged():
    return E.make_tables()["ragged"]


def _lin(ct, D, G=1, **kw):
    return dict(kind="linear", weight=np.zeros((G, ct.n_obs + D), np.float32), bias=np.zeros(G, np.float32),
                lookahead={"feature": "heat_qi", "days": D}, **kw)


def _check(ct, pol, n=4, fixes=()):
    f = P.check_linear_policy if pol["kind"] == "linear" else P.check_mlp_policy
    return f(pol, ct.n_obs, n, ct.obs_slot, "cpu", ct.feature_names, fixes, ct.slot_of.get("alerts_2wks", -1))


# ------------------------------------------------------------------ part 5: the checks
def test_linear_policy_with_lookahead_is_split_into_slots_and_tail(ct):
    D = 3
    pol = _lin(ct, D, G=2, group=np.array([0, 1, 1, 0]))
    pol["weight"] = np.arange(2 * (ct.n_obs + D), dtype=np.float32).reshape(2, -1)
    a = _check(ct, pol)
    assert (a.look_feature, a.look_days) == ("heat_qi", D)
    assert tuple(a.look_weight.shape) == (2, P.LOOKAHEAD_PAD) and a.look_weight.dtype == torch.float32
    np.testing.assert_array_equal(a.look_weight[:, :D].numpy(), pol["weight"][:, ct.n_obs:])
    assert not a.look_weight[:, D:].any()
    without = _check(ct, dict(kind="linear", weight=pol["weight"][:, :ct.n_obs], bias=pol["bias"], group=pol["group"]))
    assert torch.equal(a.weight_slots, without.weight_slots) and without.look_days == 0 and without.look_weight is None


@pytest.mark.parametrize("days", [0, 11, -1, 2.0, "3", True, None])
def test_days_outside_1_to_10_or_not_an_int_is_refused(ct, days):
    pol = _lin(ct, 3)
    pol["lookahead"] = {"feature": "heat_qi", "days": days}
    with pytest.raises(ValueError, match="lookahead"):
        _check(ct, pol)


def test_unknown_and_state_sourced_features_are_refused(ct):
    for feat in ("no_such_column", "alert_lag1", "alerts_streak", "remaining_budget"):
        if feat != "no_such_column" and feat not in ct.feature_names:
            continue
        pol = _lin(ct, 2)
        pol["lookahead"]["feature"] = feat
        with pytest.raises(ValueError, match="lookahead feature"):
            _check(ct, pol)
    state_cols = [f for f in ct.feature_names if 24 <= ct.obs_slot[ct.feature_names.index(f)] <= 27]
    assert state_cols  # the loop above met the run-time slots
    if "alerts_2wks" in ct.feature_names:  # the fix makes the column state-sourced
        pol = _lin(ct, 2)
        pol["lookahead"]["feature"] = "alerts_2wks"
        with pytest.raises(ValueError, match="table-sourced"):
            _check(ct, pol, fixes={"alert_2wks"})
    for bad in ("heat_qi", {"feature": "heat_qi"}, {"feature": "heat_qi", "days": 2, "noise": 1}):
        pol = _lin(ct, 2)
        pol["lookahead"] = bad
        with pytest.raises(ValueError, match="lookahead"):
            _check(ct, pol)


def test_weight_width_must_be_n_obs_plus_days(ct):
    for width in (ct.n_obs, ct.n_obs + 2, ct.n_obs + 4):
        pol = _lin(ct, 3)
        pol["weight"] = np.zeros((1, width), np.float32)
        with pytest.raises(ValueError, match="n_obs \\+ D"):
            _check(ct, pol)
    layers = LR.widen_net(M.net(ct, "tanh7x13", (7, 13), 1), 3, seed=1)
    g = E.groups(4) % E.G
    ok = dict(kind="mlp", layers=layers, group=g, lookahead={"feature": "heat_qi", "days": 3})
    a = _check(ct, ok)
    assert a.look_days == 3 and a.params.shape[1] == P.mlp_lookahead_stride(16, 2)
    for days in (2, 4):  # the first layer's width disagrees with the key
        with pytest.raises(ValueError, match="layer 0 weight"):
            _check(ct, dict(ok, lookahead={"feature": "heat_qi", "days": days}))
    with pytest.raises(ValueError, match="layer 0 weight"):  # ... or with there being no key
        _check(ct, {k: v for k, v in ok.items() if k != "lookahead"})
    with pytest.raises(ValueError, match="layer 1 weight"):  # inconsistent across layers
        _check(ct, dict(ok, layers=[layers[0], (layers[1][0][:, :, :-1], layers[1][1]), layers[2]]))
    with pytest.raises(ValueError, match="number of groups"):  # ... and across groups
        _check(ct, dict(ok, layers=[(layers[0][0][:3], layers[0][1][:3])] + layers[1:]))


def test_mlp_from_module_takes_the_wider_first_layer(ct):
    D = 4
    net = torch.nn.Sequential(torch.nn.Linear(ct.n_obs + D, 9), torch.nn.Tanh(), torch.nn.Linear(9, 1))
    pol = P.mlp_from_module(net)
    pol["lookahead"] = {"feature": "heat_qi", "days": D}
    a = _check(ct, pol)
    tail = a.params[0, P.mlp_stride(16, 1):].reshape(P.LOOKAHEAD_PAD, 16)
    np.testing.assert_array_equal(tail[:D, :9].numpy(), net[0].weight.detach()[:, ct.n_obs:].T.numpy())
    assert not tail[D:].any() and not tail[:, 9:].any()
    np.testing.assert_array_equal(a.params[0, :P.mlp_stride(16, 1)].numpy(), P.pack_mlp(
        [(net[0].weight.detach()[:, :ct.n_obs], net[0].bias.detach()), (net[2].weight.detach(), net[2].bias.detach())],
        ct.obs_slot, ct.n_obs)[0][0].numpy())  # nothing before the tail moves


@pytest.mark.parametrize("name", ["tanh7x13", "relu29_o2", "tanh64x33_o2"])
@pytest.mark.parametrize("D", [1, 3, 10])
def test_pack_and_unpack_are_adjoint_with_the_tail(ct, name, D):
    """<pack(L), P> = <L, unpack(P)> for random L and P (fp64 sums of the f32-representable values)."""
    _, hidden, _, n_out = M.MATRIX[name]
    rng = np.random.default_rng(D)
    L = [(np.round(W * 64) / 64, np.round(b * 64) / 64) for W, b in LR.widen_net(M.net(ct, name, hidden, n_out), D, seed=D)]
    packed, w, nl, G = P.pack_mlp(L, ct.obs_slot, ct.n_obs, D)
    assert packed.shape == (G, P.mlp_lookahead_stride(w, nl))
    Pr = torch.as_tensor(np.round(rng.standard_normal(tuple(packed.shape)) * 16) / 16, dtype=torch.float64)
    U = P.unpack_mlp_grad(Pr, ct.obs_slot, ct.n_obs, hidden, n_out, D)
    assert tuple(U[0][0].shape) == (G, hidden[0], ct.n_obs + D)
    lhs = float((packed.double() * Pr).sum())
    rhs = sum(float((torch.as_tensor(W, dtype=torch.float64) * dW).sum() + (torch.as_tensor(b, dtype=torch.float64) * db).sum())
              for (W, b), (dW, db) in zip(L, U))
    assert lhs == pytest.approx(rhs, rel=1e-12, abs=1e-9)


def test_stride_and_constants_match_the_header():
    assert int(re.search(r"#define W2A_LOOKAHEAD_MAX_DAYS (\d+)", HEADER).group(1)) == P.LOOKAHEAD_MAX_DAYS == 10
    assert int(re.search(r"#define W2A_LOOKAHEAD_PAD (\d+)", HEADER).group(1)) == P.LOOKAHEAD_PAD == 12
    m = re.search(r"#define W2A_MLP_LOOKAHEAD_STRIDE\(width, n_layers\) \((.*)\)\n", HEADER)
    assert m.group(1) == "W2A_MLP_STRIDE(width, n_layers) + W2A_LOOKAHEAD_PAD * (width)"
    for w in P.MLP_WIDTHS:
        for nl in (1, 2):
            assert P.mlp_lookahead_stride(w, nl) == P.mlp_stride(w, nl) + 12 * w
            assert P.mlp_lookahead_stride(w, nl) % 4 == 0  # blocks stay 16-B aligned


def test_abi_is_still_18_and_the_new_symbols_are_declared_and_bound():
    assert _ffi.ABI_VERSION == 18 and re.search(r"#define W2A_ABI_VERSION 18\b", HEADER)
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    binding = open(os.path.join(ROOT, "weather2alert_amd", "_ffi.py")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), s
        assert s in _ffi.SYMBOLS and f"lib.{s}.argtypes" in binding, s
    assert [n for n, _ in _ffi.Lookahead._fields_] == ["series", "stride", "days", "weight"]


def test_new_entry_points_check_the_handle_first():
    """every w2a_lookahead_* export, with a NULL handle and never-read fake pointers: W2A_ERR_ARG and its own name"""
    import ctypes as C

    from weather2alert_amd import build
    build.build_lib()
    lib = _ffi.load()
    P4 = 4096
    lin, mlp = _ffi.LinearPolicy(), _ffi.MlpPolicy()
    lin.weight = lin.bias = P4
    lin.n_groups, lin.sample = 1, 1
    mlp.params, mlp.n_groups, mlp.n_layers, mlp.width, mlp.sample = P4, 1, 2, 64, 1
    lk = _ffi.Lookahead()
    lk.series, lk.stride, lk.days, lk.weight = P4, 153, 3, P4
    roll = (5, P4, P4, P4, P4, None, None, 0, P4, None, None, C.byref(lk))
    calls = {"w2a_lookahead_rollout_linear": (C.byref(lin),) + roll,
             "w2a_lookahead_rollout_linear_gated": (C.byref(lin),) + roll + (P4, 5),
             "w2a_lookahead_rollout_mlp": (C.byref(mlp),) + roll,
             "w2a_lookahead_rollout_mlp_gated": (C.byref(mlp),) + roll + (P4, 5),
             "w2a_lookahead_policy_gradient_linear": (C.byref(lin), 0, 5, P4, P4, P4, 1 << 20, None, C.byref(lk), None, 0),
             "w2a_lookahead_imitation_gradient_linear": (C.byref(lin), P4, 5, None, None, 0, 5, P4, P4, P4, P4, None,
                                                         C.byref(lk), None, 0)}
    assert set(calls) == set(NEW_SYMBOLS)
    for name, args in calls.items():
        assert getattr(lib, name)(None, *args) == -1, name
        assert lib.w2a_last_error().decode() == f"{name}: NULL handle", name


# ------------------------------------------------------------------ part 6: the refusals
def _bare_env(ct, n=4):
    """An env object no device ever saw: every refusal below is raised before anything else is read."""
    env = object.__new__(HeatAlertVecEnv)
    env.ct, env.num_envs, env.device, env.fixes, env.reward_mode = ct, n, torch.device("cpu"), set(), "sampled"
    env._needs_reset, env._pm = False, False
    return env


def test_entry_points_that_do_not_take_lookahead_say_so(ct):
    n = 4
    env = _bare_env(ct, n)
    lin = _lin(ct, 3, sample=True)
    mlp = dict(kind="mlp", layers=[(np.zeros((5, ct.n_obs + 3), np.float32), np.zeros(5, np.float32)),
                                   (np.zeros((2, 5), np.float32), np.zeros(2, np.float32))],
               sample=True, lookahead={"feature": "heat_qi", "days": 3})
    days = np.zeros((n, ct.T), bool)
    adv = np.zeros((ct.T, n), np.float32)
    with pytest.raises(ValueError, match=r"rollout\(record=True\).*lookahead"):
        env.rollout(lin, record=True)
    with pytest.raises(ValueError, match=r"rollout\(record=True\).*lookahead"):
        env.rollout(mlp, record=True)
    with pytest.raises(ValueError, match=r"rollout\(policy_gradient=\.\.\.\).*lookahead"):
        env.rollout(mlp, policy_gradient="none")
    with pytest.raises(ValueError, match=r"imitation_gradient\(\).*lookahead"):
        env.imitation_gradient(mlp, days)
    for pol in (lin, mlp):
        with pytest.raises(ValueError, match=r"surrogate_gradient\(\).*lookahead"):
            env.surrogate_gradient(pol, days, adv)
        with pytest.raises(ValueError, match=r"fisher_vector_product\(\).*lookahead"):
            env.fisher_vector_product(pol, days, {})
        with pytest.raises(ValueError, match=r"value_gradient\(\).*lookahead"):
            env.value_gradient(pol, days)
    with pytest.raises(ValueError, match=r"q_gradient\(\).*lookahead"):
        env.q_gradient(mlp, days)
    with pytest.raises(ValueError, match=r"q_gradient\(\).*lookahead"):
        env.q_gradient({k: v for k, v in mlp.items() if k != "lookahead"}, days, target_net=mlp)


# ------------------------------------------------------------------ the restatement alone
def test_inputs_are_zero_from_the_envs_own_last_day_on(ragged):
    ct = ragged.ct
    h = LR.series(ct, "heat_qi")
    R = ct.S_w * ct.Y
    cw, yi = np.divmod(np.arange(R), ct.Y)
    nd = ct.n_days[np.arange(R)].astype(np.int64)
    assert len(np.unique(nd)) > 10 and nd.min() == 1  # ragged, the one-day episode included
    D = 10
    for back in range(0, 13):  # held rows counted from each episode's end
        t = np.maximum(nd - back, 0)  # r = max(t - 1, 0)
        f = LR.inputs(ct, "heat_qi", D, dict(t=t, n_days=nd, county_w=cw, year_i=yi))
        r = LR.held_day(t)
        for k in range(1, D + 1):
            past = r + k >= nd
            assert not f[past, k - 1].any()
            np.testing.assert_array_equal(f[~past, k - 1], h[np.arange(R)[~past], (r + k)[~past]] - h[np.arange(R)[~past], r[~past]])
    assert h.dtype == np.float32 and f.dtype == np.float32


def test_the_first_two_decisions_of_an_episode_hold_row_zero(ct):
    R = ct.S_w * ct.Y
    cw, yi = np.divmod(np.arange(R), ct.Y)
    nd = ct.n_days[np.arange(R)].astype(np.int64)
    st = dict(n_days=nd, county_w=cw, year_i=yi)
    f0 = LR.inputs(ct, "heat_qi", 3, dict(st, t=np.zeros(R, np.int64)))
    f1 = LR.inputs(ct, "heat_qi", 3, dict(st, t=np.ones(R, np.int64)))
    f2 = LR.inputs(ct, "heat_qi", 3, dict(st, t=np.full(R, 2)))
    np.testing.assert_array_equal(f0, f1)
    assert (LR.held_day([0, 1, 2, 3]) == [0, 0, 1, 2]).all()
    assert (f1 != f2).any() and f0.any()


def test_weather_only_threshold_sits_between_two_table_values(ct):
    """the bias of tests/test_lookahead_gpu.py's exact test: halfway between two neighbouring distinct values of
    h(r + 1) - h(r), so no logit of that test can be a tie"""
    h = LR.series(ct, "heat_qi")
    d = np.unique((h[:, 1:] - h[:, :-1]).astype(np.float32))
    c = LR.midpoint_threshold(ct, "heat_qi")
    assert len(d) > 10 and d.min() < c < d.max() and not (d == c).any()
    gap = np.abs(d.astype(np.float64) - c).min()
    assert gap > 1e-6 * max(abs(c), 1e-3)  # far from a rounding of the fp64 sum f - c


# ------------------------------------------------------------------ the cases of the GPU file, on the host oracle alone
@pytest.fixture(scope="module")
def walk_tables():
    tb = C.make_tables()
    return {k: v + (C.host_tuples(k, v),) for k, v in tb.items()}


def _walk(walk_tables, table, pol, D, kind, sample, gate=None):
    """lookahead_restatement.host_walk over a whole episode of the GPU test's batch: the decision step is twin_loop's"""
    ct, _, oracle, tup = walk_tables[table]
    uni = LR.policy_uniform(C.SEED, C.GID0, {"episode_no": np.zeros(C.N, np.int64)}) if sample else None
    acc = LR.host_walk(oracle(), ct, tup, C.spec(D), C.logit_fn(pol), ct.T, kind, uniform=uni, gate=gate)
    # a policy that decides: alerts are issued, and not on every day (tests/test_linear_policy_gpu.py)
    assert acc["alerts"].sum() > 0 and (acc["alerts"] < tup["n_days"]).any() and acc["att"].any()
    return acc, ct, tup


@pytest.mark.parametrize("table,D,sample", C.LINEAR_CASES)
def test_linear_cases_stay_under_the_near_tie_cap(walk_tables, table, D, sample):
    acc, ct, _ = _walk(walk_tables, table, C.linear(ct_of(walk_tables, table), D, sample), D, "linear", sample)
    print(f"linear {table} D={D} sample={sample}: near-tie envs {acc['tie'].sum()} of {C.N}")
    assert acc["tie"].mean() < LR.TIE_CAP, acc["tie"].sum()


def ct_of(walk_tables, table):
    return walk_tables[table][0]


@pytest.mark.parametrize("name,D,sample", C.MLP_CASES)
def test_mlp_cases_stay_under_the_near_tie_cap(walk_tables, name, D, sample):
    table = C.mlp_table(D)
    acc, _, _ = _walk(walk_tables, table, C.mlp(ct_of(walk_tables, table), name, D, sample), D, "mlp", sample)
    print(f"mlp {name} {table} D={D} sample={sample}: near-tie envs {acc['tie'].sum()} of {C.N}")
    assert acc["tie"].mean() < LR.TIE_CAP, acc["tie"].sum()


def test_mlp_cases_reach_all_six_instantiations():
    assert {M.MATRIX[n][0] for n, _, _ in C.MLP_CASES} == {(w, l) for w in (16, 32, 64) for l in (1, 2)}


@pytest.mark.parametrize("kind,D", C.GATE_CASES)
def test_gate_cases_stay_under_the_near_tie_cap(walk_tables, kind, D):
    from alert_gate_restatement import gate_fp32

    ct, _, _, tup = walk_tables["ragged"]
    zero = np.zeros(C.N, np.int64)
    start = dict(t=zero, n_days=tup["n_days"], county_w=tup["county_w"], year_i=tup["year_i"], finished=zero)
    gate = gate_fp32(ct.X, ct.Y, ct.obs_slot[ct.feature_names.index(C.FEATURE)], start, C.GATE_THRESHOLD)
    assert gate.any() and not gate[np.arange(ct.T)[None, :] < tup["n_days"][:, None]].all()
    pol = C.linear(ct, D) if kind == "linear" else C.mlp(ct, C.GATE_NET, D)
    acc, _, _ = _walk(walk_tables, "ragged", pol, D, kind, False, gate=gate)
    assert not (acc["att"] & ~gate).any()
    assert acc["tie"].mean() < LR.TIE_CAP, acc["tie"].sum()


@pytest.mark.parametrize("table,D", C.GRADIENT_CASES)
def test_gradient_cases_meet_no_near_tie_at_all(walk_tables, table, D):
    """the group means of the gradient tests hold every env: the sampled policies of those cases draw no u within the
    bound of any sigmoid, over the whole episode"""
    acc, _, _ = _walk(walk_tables, table, C.linear(ct_of(walk_tables, table), D, sample=True), D, "linear", True)
    assert not acc["tie"].any(), acc["tie"].sum()
