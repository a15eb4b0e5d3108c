"""policy["lookahead"] = {..., "error": e, "error_seed": s} on the host: the checks of weather2alert_amd/policy.py, the
refusals of the env's entry points with the key present (every one raised before anything touches a device), the
header's struct and symbols, and the restatement alone (tests/forecast_error_restatement.py): the statistics of its
draws, its exact fma, the zero row, the end of the summer, and the cases of the GPU file walked on the host oracle."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import forecast_error_cases as FC
import forecast_error_restatement as FR
import lookahead_cases as C
import lookahead_restatement as LR
import table_edges as E
from oracle import heatalert_oracle as O
from weather2alert_amd import HeatAlertVecEnv, _ffi, policy as P, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = open(os.path.join(ROOT, "include", "w2a.h")).read()
NEW_SYMBOLS = ("w2a_forecast_rollout_linear", "w2a_forecast_rollout_mlp", "w2a_forecast_policy_gradient_linear",
               "w2a_forecast_imitation_gradient_linear", "w2a_forecast_features")


@pytest.fixture(scope="module")
def ct():
    return tables.CompiledTables.load_npz(os.path.join(GOLDEN, "mini_compiled.npz"))


@pytest.fixture(scope="module")
def ragged():
    return E.make_tables()["ragged"]


def _lin(ct, D, error, G=1, **kw):
    la = {"feature": "heat_qi", "days": D, "error": error}
    la.update({k: kw.pop(k) for k in list(kw) if k == "error_seed"})
    return dict(kind="linear", weight=np.zeros((G, ct.n_obs + D), np.float32), bias=np.zeros(G, np.float32),
                lookahead=la, **kw)


def _mlp(ct, D, **la):
    return dict(kind="mlp", layers=[(np.zeros((5, ct.n_obs + D), np.float32), np.zeros(5, np.float32)),
                                    (np.zeros((2, 5), np.float32), np.zeros(2, np.float32))],
                sample=True, lookahead=dict({"feature": "heat_qi", "days": D}, **la))


def _check(ct, pol, n=4):
    f = P.check_linear_policy if pol["kind"] == "linear" else P.check_mlp_policy
    return f(pol, ct.n_obs, n, ct.obs_slot, "cpu", ct.feature_names, (), ct.slot_of.get("alerts_2wks", -1))


# ------------------------------------------------------------------ the checks
def test_error_and_seed_travel_on_the_checked_policy(ct):
    a = _check(ct, _lin(ct, 3, 0.25))
    assert a.look_error == (0.25, 0.25, 0.25) and a.look_error_seed == 0 and a.look_days == 3
    a = _check(ct, _lin(ct, 3, [0.1, 0, np.float32(2.5)], error_seed=2**63 - 1))
    assert a.look_error == (float(np.float32(0.1)), 0.0, 2.5) and a.look_error_seed == 2**63 - 1
    a = _check(ct, _lin(ct, 2, np.array([1, 2])))
    assert a.look_error == (1.0, 2.0)
    a = _check(ct, _lin(ct, 2, torch.tensor([0.5, 1.5]), error_seed=np.int64(7)))
    assert a.look_error == (0.5, 1.5) and a.look_error_seed == 7
    m = _check(ct, _mlp(ct, 3, error=(0.5, 1, 1.5), error_seed=9))
    assert m.look_error == (0.5, 1.0, 1.5) and m.look_error_seed == 9 and m.look_days == 3
    for pol in (_lin(ct, 3, 0.25), _mlp(ct, 3, error=0.25)):  # what check_lookahead returns does not change
        assert P.check_lookahead(pol, "t", ct.feature_names, ct.obs_slot, ct.n_obs) == ("heat_qi", 3)
    assert P.check_forecast_error(_lin(ct, 3, 0.25), "t") == ((0.25,) * 3, 0)
    plain = dict(_lin(ct, 3, 0.25), lookahead={"feature": "heat_qi", "days": 3})
    assert P.check_forecast_error(plain, "t") is None and P.check_forecast_error({"kind": "linear"}, "t") is None
    a = _check(ct, plain)
    assert a.look_error is None and a.look_error_seed == 0


@pytest.mark.parametrize("error", [True, False, "0.2", None, -0.1, float("nan"), float("inf"), 1e39, [0.1, 0.2],
                                   [0.1, 0.2, 0.3, 0.4], [0.1, -0.2, 0.3], [0.1, float("nan"), 0.3], [0.1, True, 0.3],
                                   [0.1, "0.2", 0.3], [0.1, None, 0.3], [], {"mae": 1}, np.zeros((3, 1)), b"abc"])
def test_bad_error_values_are_refused(ct, error):
    for pol in (_lin(ct, 3, error), _mlp(ct, 3, error=error)):
        with pytest.raises(ValueError, match="lookahead"):
            _check(ct, pol)


@pytest.mark.parametrize("seed", [-1, 2**63, 1.0, "1", True, None])
def test_bad_error_seeds_are_refused(ct, seed):
    with pytest.raises(ValueError, match="lookahead"):
        _check(ct, _lin(ct, 3, 0.2, error_seed=seed))


def test_seed_without_error_and_unknown_keys_are_refused(ct):
    for la in ({"feature": "heat_qi", "days": 3, "error_seed": 1},
               {"feature": "heat_qi", "days": 3, "error": 0.2, "noise": 1},
               {"feature": "heat_qi", "days": 3, "noise": 1},
               {"feature": "heat_qi", "error": 0.2},
               {"feature": "heat_qi", "days": 3, "error": 0.2, "error_seed": 1, "seed": 2}):
        pol = _lin(ct, 3, 0.2)
        pol["lookahead"] = la
        with pytest.raises(ValueError, match="lookahead"):
            _check(ct, pol)


# ------------------------------------------------------------------ the refusals of test_lookahead_cpu.py part 6, with "error"
def _bare_env(ct, n=4):
    """An env object no device ever saw: every refusal below is raised before anything else is read."""
    env = object.__new__(HeatAlertVecEnv)
    env.ct, env.num_envs, env.device, env.fixes, env.reward_mode = ct, n, torch.device("cpu"), set(), "sampled"
    env._needs_reset, env._pm = False, False
    return env


def test_entry_points_that_do_not_take_lookahead_refuse_it_with_error_too(ct):
    n = 4
    env = _bare_env(ct, n)
    lin = _lin(ct, 3, 0.2, sample=True, error_seed=4)
    mlp = _mlp(ct, 3, error=[0.1, 0.2, 0.3])
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
    with pytest.raises(ValueError, match=r"imitation_gradient\(labels=\.\.\.\).*lookahead"):
        env.imitation_gradient(lin, days, labels=days)
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
    with pytest.raises(ValueError, match="lookahead"):
        env.policy_budget_curve(lin, 3)
    # a bad value is refused by the entry points that do take the key, before a device is touched
    for bad in (dict(lin, lookahead=dict(lin["lookahead"], error=-1.0)),
                dict(lin, lookahead={"feature": "heat_qi", "days": 3, "error_seed": 1})):
        with pytest.raises(ValueError, match="lookahead"):
            env.rollout(bad)
        with pytest.raises(ValueError, match="lookahead"):
            env.rollout(bad, policy_gradient="none")
        with pytest.raises(ValueError, match="lookahead"):
            env.imitation_gradient(bad, days)
        with pytest.raises(ValueError, match="lookahead"):
            env.lookahead_features(bad["lookahead"])


# ------------------------------------------------------------------ the ABI
def test_abi_is_still_18_and_the_new_struct_and_symbols_are_declared_and_bound():
    assert _ffi.ABI_VERSION == 18 and re.search(r"#define W2A_ABI_VERSION 18\b", HEADER)
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    binding = open(os.path.join(ROOT, "weather2alert_amd", "_ffi.py")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), s
        assert s in _ffi.SYMBOLS and f"lib.{s}.argtypes" in binding, s
    m = re.search(r"typedef struct w2a_forecast_error \{(.*?)\} w2a_forecast_error;", code, flags=re.S)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == ["float mae[W2A_LOOKAHEAD_PAD]", "uint64_t seed"]
    assert [n for n, _ in _ffi.ForecastError._fields_] == ["mae", "seed"]
    assert ctypes.sizeof(_ffi.ForecastError) == 4 * P.LOOKAHEAD_PAD + 8
    assert [n for n, _ in _ffi.Lookahead._fields_] == ["series", "stride", "days", "weight"]  # unchanged
    assert "0xC3C3C3C33C3C3C3C" in HEADER and FR.NOISE_C == 0xC3C3C3C33C3C3C3C  # the counter formula is in the header


def test_new_entry_points_check_the_handle_first():
    """every w2a_forecast_* export, with a NULL handle and never-read fake pointers: W2A_ERR_ARG and its own name"""
    from weather2alert_amd import build
    build.build_lib()
    lib = _ffi.load()
    Cb = ctypes.byref
    P4 = 4096
    lin, mlp = _ffi.LinearPolicy(), _ffi.MlpPolicy()
    lin.weight = lin.bias = P4
    lin.n_groups, lin.sample = 1, 1
    mlp.params, mlp.n_groups, mlp.n_layers, mlp.width, mlp.sample = P4, 1, 2, 64, 1
    lk = _ffi.Lookahead()
    lk.series, lk.stride, lk.days, lk.weight = P4, 153, 3, P4
    fe = _ffi.ForecastError()
    fe.mae[0], fe.seed = 0.5, 3
    roll = (5, P4, P4, P4, P4, None, None, 0, P4, None, None, Cb(lk))
    calls = {"w2a_forecast_rollout_linear": [(Cb(lin),) + roll + (None, 0, Cb(fe)), (Cb(lin),) + roll + (P4, 5, Cb(fe))],
             "w2a_forecast_rollout_mlp": [(Cb(mlp),) + roll + (None, 0, Cb(fe)), (Cb(mlp),) + roll + (P4, 5, Cb(fe))],
             "w2a_forecast_policy_gradient_linear": [(Cb(lin), 0, 5, P4, P4, P4, 1 << 20, None, Cb(lk), None, 0, Cb(fe))],
             "w2a_forecast_imitation_gradient_linear": [(Cb(lin), P4, 5, None, None, 0, 5, P4, P4, P4, P4, None, Cb(lk),
                                                         None, 0, Cb(fe))],
             "w2a_forecast_features": [(Cb(lk), Cb(fe), P4, None)]}
    assert set(calls) == set(NEW_SYMBOLS)
    for name, variants in calls.items():
        for args in variants:
            assert getattr(lib, name)(None, *args) == -1, name
            assert lib.w2a_last_error().decode() == f"{name}: NULL handle", name


# ------------------------------------------------------------------ the restatement alone: the draws
SEED_A, SEED_B = 11, 12  # two error seeds; the policies' SEED = lookahead_cases.SEED
N_ENV, N_DAY, N_LEAD = 64, 153, 10  # 97 920 (env, day, lead) triples


def _draws(seed, gid0=C.GID0):
    st = FR.stream(seed, gid0 + np.arange(N_ENV), np.zeros(N_ENV, np.int64))
    return FR.uniform(st[:, None, None], np.arange(N_DAY)[None, :, None], np.arange(1, N_LEAD + 1)[None, None, :])


def _corr(a, b):
    return float(np.corrcoef(np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel())[0, 1])


def test_draws_are_uniform_on_minus_one_to_one_and_uncorrelated():
    u = _draws(SEED_A)
    assert u.dtype == np.float32 and u.shape == (N_ENV, N_DAY, N_LEAD) and u.size >= 97_000
    assert u.min() >= -1.0 and u.max() < 1.0
    assert ((u.astype(np.float64) + 1.0) * 2.0 ** 23 % 1 == 0).all()  # 24-bit values, exact in f32
    x = u.astype(np.float64)
    se = np.sqrt(1.0 / 3.0 / x.size)
    figures = dict(mean_over_se=x.mean() / se, var=x.var(), leads=_corr(x[:, :, :-1], x[:, :, 1:]),
                   days=_corr(x[:, :-1, :], x[:, 1:, :]), envs=_corr(x[:-1], x[1:]), seeds=_corr(x, _draws(SEED_B)),
                   halves=_corr(x[:, :, 0::2], x[:, :, 1::2]))
    # the Bernoulli uniforms of the policy with the SAME seed, on the same (env, day)
    pu = O.devrng_policy_uniform_vec(SEED_A, (C.GID0 + np.arange(N_ENV))[:, None], np.zeros((N_ENV, 1), np.int64),
                                     np.arange(N_DAY)[None, :])
    figures["policy"] = max(abs(_corr(x[:, :, k], pu)) for k in range(N_LEAD))
    print(figures)
    assert abs(figures["mean_over_se"]) <= 4
    assert abs(figures["var"] - 1.0 / 3.0) <= 0.02 / 3.0
    for k in ("leads", "days", "envs", "seeds", "halves", "policy"):
        assert abs(figures[k]) < 0.02, (k, figures[k])


def test_draws_depend_on_seed_global_id_episode_day_and_lead_only():
    a = _draws(SEED_A, gid0=C.GID0)
    b = _draws(SEED_A, gid0=C.GID0 + 5)
    np.testing.assert_array_equal(a[5:], b[:-5])  # the global id, not the position in the batch
    st0 = FR.stream(SEED_A, C.GID0 + np.arange(4), np.zeros(4, np.int64))
    st1 = FR.stream(SEED_A, C.GID0 + np.arange(4), np.ones(4, np.int64))
    assert len(set(st0.tolist()) | set(st1.tolist())) == 8  # another episode, another stream
    # the scalar statement of the header, with Python integers
    M = 2**64 - 1
    for gid, ep, r, k in [(C.GID0, 0, 0, 1), (C.GID0 + 3, 2, 17, 2), (7, 1, 152, 9), (7, 1, 152, 10)]:
        st = O.devrng_stream(SEED_A ^ FR.NOISE_C, gid, ep)
        x = O._mix64((st + (8 * r + ((k - 1) >> 1) + 1) * 0x9E3779B97F4A7C15) & M)
        word = x >> 32 if k & 1 else x & 0xFFFFFFFF
        want = np.float32(word >> 8) * np.float32(2.0 ** -23) - np.float32(1)
        got = FR.uniform(FR.stream(SEED_A, np.array([gid]), np.array([ep])), np.array([r]), k)[0]
        assert got == want


def test_the_restatements_fma_rounds_once():
    rng = np.random.default_rng(5)
    n = 4000
    a = (rng.random(n) * 2 - 1).astype(np.float32)
    b = np.float32(7.0) * rng.random(n).astype(np.float32)
    c = (rng.standard_normal(n) * np.exp(rng.uniform(-30, 3, n))).astype(np.float32)
    # cases where rounding the f64 sum first lands on a halfway point of f32 whose even neighbour is the wrong one:
    # c = 1 + 2^-23 (odd), a * b = 2^-24 (1 - 2^-46): the exact sum lies just below the halfway point
    a = np.concatenate([a, np.float32([1 + 2.0 ** -23, 1 + 2.0 ** -23])])
    b = np.concatenate([b, np.float32([2.0 ** -24 * (1 - 2.0 ** -23), -(2.0 ** -24) * (1 - 2.0 ** -23)])])
    c = np.concatenate([c, np.float32([1 + 2.0 ** -23, -(1 + 2.0 ** -23)])])
    got = FR.fma32(a, b, c)

    def exact(x, y, z):
        v = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.float32(float(v))  # may be off by one f32 step (two roundings): pick the nearest of its neighbours
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda q: (abs(Fraction(float(q)) - v), int(q.view(np.uint32)) & 1))
        return best

    want = np.array([exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (naive[-2:] != want[-2:]).all()  # the crafted cases are ones two roundings get wrong


# ------------------------------------------------------------------ the restatement alone: the inputs
def _all_rows(ct):
    R = ct.S_w * ct.Y
    cw, yi = np.divmod(np.arange(R), ct.Y)
    return R, dict(n_days=ct.n_days[np.arange(R)].astype(np.int64), county_w=cw, year_i=yi)


@pytest.mark.parametrize("zero", [0, 0.0, [0.0] * 10, np.zeros(10, np.float32)])
def test_zero_error_gives_the_bits_of_the_clean_restatement(ragged, zero):
    ct = ragged.ct
    R, st = _all_rows(ct)
    for t in (0, 1, 5, 40):
        s = dict(st, t=np.minimum(t, st["n_days"] - 1))
        f = FR.inputs(ct, dict(feature="heat_qi", days=10, error=zero, error_seed=3), s, C.GID0)
        np.testing.assert_array_equal(f.view(np.uint32), LR.inputs(ct, "heat_qi", 10, s).view(np.uint32))
    # ... for every finite h: a -0 in the table stays a -0 (an fma with a zero MAE would make it +0)
    fake = type("T", (), dict(X=np.zeros((4, 1, 32), np.float32), Y=1, obs_slot=list(range(32)), feature_names=["heat_qi"]))
    fake.X[1:, 0, 0] = [-0.0, 0.0, -0.0]
    s = dict(t=np.array([0]), n_days=np.array([4]), county_w=np.array([0]), year_i=np.array([0]))
    f = FR.inputs(fake, dict(feature="heat_qi", days=3, error=0.0), s, 0)
    np.testing.assert_array_equal(f.view(np.uint32), LR.inputs(fake, "heat_qi", 3, s).view(np.uint32))
    assert np.signbit(f[0, 0]) and not np.signbit(f[0, 1])


def test_inputs_past_the_end_are_plus_zero_and_the_noise_is_bounded(ragged):
    ct = ragged.ct
    R, st = _all_rows(ct)
    nd = st["n_days"]
    D = 10
    spec = FC.spec(D)
    e = FR.error_row(spec["error"], D)
    moved = 0
    for back in range(0, 13):
        s = dict(st, t=np.maximum(nd - back, 0))
        f, f0 = FR.inputs(ct, spec, s, C.GID0), LR.inputs(ct, "heat_qi", D, s)
        r = LR.held_day(s["t"])
        for k in range(1, D + 1):
            past = r + k >= nd
            assert (f[past, k - 1].view(np.uint32) == 0).all()  # +0 exactly, no noise
            d = np.abs(f[~past, k - 1].astype(np.float64) - f0[~past, k - 1])
            ulp = np.spacing(np.maximum(np.abs(f[~past, k - 1]), np.abs(f0[~past, k - 1])).astype(np.float32))
            assert (d <= e[k - 1] + 2.0 * ulp).all()
            moved += int((d > 0).sum())
    assert f.dtype == np.float32 and moved > 1000
    # h(r) itself is exact: with the error on one lead only, the other leads are the clean ones
    one = dict(spec, error=[0.0] * 4 + [0.2] + [0.0] * 5)
    s = dict(st, t=np.minimum(3, nd - 1))
    f, f0 = FR.inputs(ct, one, s, C.GID0), LR.inputs(ct, "heat_qi", D, s)
    np.testing.assert_array_equal(np.delete(f, 4, axis=1), np.delete(f0, 4, axis=1))
    assert (f[:, 4] != f0[:, 4]).any()


def test_episode_number_and_seed_move_the_inputs(ct):
    R, st = _all_rows(ct)
    s = dict(st, t=np.full(R, 9))
    spec = FC.spec(3)
    a = FR.inputs(ct, spec, s, C.GID0)
    np.testing.assert_array_equal(a, FR.inputs(ct, spec, dict(s, episode_no=np.zeros(R, np.int64)), C.GID0))
    assert (a != FR.inputs(ct, spec, dict(s, episode_no=np.ones(R, np.int64)), C.GID0)).mean() > 0.9
    assert (a != FR.inputs(ct, dict(spec, error_seed=spec["error_seed"] + 1), s, C.GID0)).mean() > 0.9
    assert (a != FR.inputs(ct, spec, s, C.GID0 + 1)).mean() > 0.9


# ------------------------------------------------------------------ the cases of the GPU file, on the host oracle alone
@pytest.fixture(scope="module")
def walk_tables():
    tb = C.make_tables()
    return {k: v + (C.host_tuples(k, v),) for k, v in tb.items()}


def _walk(walk_tables, table, pol, kind, sample, gate=None):
    ct, _, oracle, tup = walk_tables[table]
    uni = LR.policy_uniform(C.SEED, C.GID0, {"episode_no": np.zeros(C.N, np.int64)}) if sample else None
    acc = FR.host_walk(oracle(), ct, tup, pol["lookahead"], C.GID0, C.logit_fn(pol), ct.T, kind, uniform=uni, gate=gate)
    assert acc["alerts"].sum() > 0 and (acc["alerts"] < tup["n_days"]).any() and acc["att"].any()  # a policy that decides
    clean = LR.host_walk(oracle(), ct, tup, FR.clean(pol["lookahead"]), C.logit_fn(pol), ct.T, kind, uniform=uni, gate=gate)
    assert (acc["days"] != clean["days"]).any()  # ... and the error is not vacuous: it moves decisions
    return acc


@pytest.mark.parametrize("table,D,sample,row", FC.LINEAR_CASES)
def test_linear_cases_meet_no_near_tie(walk_tables, table, D, sample, row):
    ct = walk_tables[table][0]
    acc = _walk(walk_tables, table, FC.linear(ct, D, sample, row, key=("linear", table, D)), "linear", sample)
    assert not acc["tie"].any(), acc["tie"].sum()


@pytest.mark.parametrize("name,D,sample", FC.MLP_CASES)
def test_mlp_cases_meet_no_near_tie(walk_tables, name, D, sample):
    table = C.mlp_table(D)
    ct = walk_tables[table][0]
    acc = _walk(walk_tables, table, FC.mlp(ct, name, D, sample, key=("mlp", name, D)), "mlp", sample)
    assert not acc["tie"].any(), acc["tie"].sum()


def test_mlp_cases_reach_all_six_instantiations_and_the_k_step_boundaries():
    import policy_gradient_mlp_cases as M
    assert {M.MATRIX[n][0] for n, _, _ in FC.MLP_CASES} == {(w, l) for w in (16, 32, 64) for l in (1, 2)}
    assert {D for _, D, _ in FC.MLP_CASES} == {4, 5, 10}


@pytest.mark.parametrize("kind,D", FC.GATE_CASES)
def test_gate_cases_meet_no_near_tie(walk_tables, kind, D):
    from alert_gate_restatement import gate_fp32

    ct, _, _, tup = walk_tables["ragged"]
    zero = np.zeros(C.N, np.int64)
    start = dict(t=zero, n_days=tup["n_days"], county_w=tup["county_w"], year_i=tup["year_i"], finished=zero)
    gate = gate_fp32(ct.X, ct.Y, ct.obs_slot[ct.feature_names.index(C.FEATURE)], start, C.GATE_THRESHOLD)
    pol = FC.linear(ct, D, key=("gate", kind, D)) if kind == "linear" else FC.mlp(ct, FC.GATE_NET, D, key=("gate", kind, D))
    acc = _walk(walk_tables, "ragged", pol, kind, False, gate=gate)
    assert not (acc["att"] & ~gate).any() and not acc["tie"].any(), acc["tie"].sum()


@pytest.mark.parametrize("table,D", FC.GRADIENT_CASES)
def test_gradient_cases_meet_no_near_tie(walk_tables, table, D):
    ct = walk_tables[table][0]
    acc = _walk(walk_tables, table, FC.linear(ct, D, sample=True, key=("gradient", table, D)), "linear", True)
    assert not acc["tie"].any(), acc["tie"].sum()
