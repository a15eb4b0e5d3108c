"""policy["lookahead"] on other observation layouts, on the host alone: every rollout case of
tests/lookahead_layout_cases.py walked on the vector oracle (lookahead_restatement.host_walk) -- the near-tie cap, and
that the lookahead inputs decide something (the same policy with its lookahead columns zeroed attempts other days in at
least one env of ten) -- the placement of every weight by check_linear_policy / pack_mlp / unpack_mlp_grad at D on both
sides of a k-step of four, and check_lookahead on every column name of two layouts."""
import numpy as np
import pytest
import torch

import lookahead_cases as C
import lookahead_layout_cases as K
import lookahead_restatement as LR
import policy_gradient_mlp_cases as M
from weather2alert_amd import policy as P

SENSITIVE_SHARE = 0.1  # envs whose attempt bitmap must change when the lookahead columns are zeroed


@pytest.fixture(scope="module")
def tabs():
    return K.make_tables()


@pytest.fixture(scope="module")
def tuples(tabs):
    return {name: K.host_tuples(tb) for name, tb in tabs.items()}


def _walk(tb, tup, pol, kind, gate=None):
    ct, la = tb.ct, pol["lookahead"]
    uni = K.uniform(tb.name) if pol["sample"] else None
    return LR.host_walk(tb.oracle(), ct, tup, la, C.logit_fn(pol), ct.T, kind, uniform=uni, gate=gate)


def _conditions(tb, tup, pol, kind, what, gate=None):
    """the two input conditions of a rollout case; prints the figures before it asserts"""
    acc = _walk(tb, tup, pol, kind, gate)
    off = _walk(tb, tup, K.zeroed(pol, tb.ct), kind, gate)
    changed = (acc["att"] != off["att"]).any(axis=1)
    print(f"{what}: near-tie envs {acc['tie'].sum()} of {K.N}, envs with alerts {(acc['alerts'] > 0).sum()}, envs whose "
          f"attempts depend on the lookahead columns {changed.sum()}")
    # a policy that decides: alerts are issued, and not on every day (tests/test_linear_policy_gpu.py)
    assert acc["alerts"].sum() > 0 and (acc["alerts"] < tup["n_days"]).any() and acc["att"].any()
    assert acc["tie"].mean() < LR.TIE_CAP, acc["tie"].sum()
    assert changed.mean() >= SENSITIVE_SHARE, changed.sum()
    return acc


# ------------------------------------------------------------------ the rollout cases, on the host oracle alone
@pytest.mark.parametrize("table,feature,D,sample", K.LINEAR_CASES)
def test_linear_cases_meet_the_input_conditions(tabs, tuples, table, feature, D, sample):
    tb = tabs[table]
    _conditions(tb, tuples[table], K.linear(tb, feature, D, sample), "linear", f"linear {table} {feature} D={D} sample={sample}")


@pytest.mark.parametrize("table,feature,D,sample,net", K.MLP_CASES)
def test_mlp_cases_meet_the_input_conditions(tabs, tuples, table, feature, D, sample, net):
    tb = tabs[table]
    _conditions(tb, tuples[table], K.mlp(tb, feature, net, D, sample), "mlp", f"mlp {net} {table} {feature} D={D} sample={sample}")


def test_mlp_cases_cover_what_the_gpu_file_promises():
    assert {M.MATRIX[n][0] for *_, n in K.MLP_CASES} == {(w, l) for w in (16, 32, 64) for l in (1, 2)}
    assert {D for _, _, D, _, _ in K.MLP_CASES} >= {2, 4, 5, 8, 9}
    assert {t for t, *_ in K.MLP_CASES} >= {"permuted", "n28", "n8", "narrow", "n8_ragged", "ragged27"}
    assert sum(f != "heat_qi" for _, f, *_ in K.MLP_CASES) >= 2


@pytest.mark.parametrize("kind,table,feature,D,gate_feature,net", K.GATE_CASES)
def test_gate_cases_meet_the_input_conditions(tabs, tuples, kind, table, feature, D, gate_feature, net):
    from alert_gate_restatement import gate_fp32

    tb, tup = tabs[table], tuples[table]
    ct = tb.ct
    assert gate_feature != feature
    zero = np.zeros(K.N, np.int64)
    start = dict(t=zero, n_days=tup["n_days"], county_w=tup["county_w"], year_i=tup["year_i"], finished=zero)
    gate = gate_fp32(ct.X, ct.Y, ct.obs_slot[ct.feature_names.index(gate_feature)], start, K.gate_threshold(ct, gate_feature))
    assert gate.any() and not gate[np.arange(ct.T)[None, :] < tup["n_days"][:, None]].all()
    pol = K.linear(tb, feature, D) if kind == "linear" else K.mlp(tb, feature, net, D)
    acc = _conditions(tb, tup, pol, kind, f"gated {kind} {table} D={D}", gate=gate)
    assert not (acc["att"] & ~gate).any()


@pytest.mark.parametrize("table,feature,D", K.GRADIENT_CASES)
def test_gradient_cases_meet_no_near_tie_at_all(tabs, tuples, table, feature, D):
    """the group means of the gradient tests hold every env: the sampled policies of those cases draw no u within the
    bound of any sigmoid, over the whole episode"""
    tb = tabs[table]
    acc = _walk(tb, tuples[table], K.linear(tb, feature, D, sample=True), "linear")
    assert acc["alerts"].sum() > 0 and not acc["tie"].any(), acc["tie"].sum()


@pytest.mark.parametrize("table,feature,D,k", K.WEATHER_RULE_CASES)
def test_weather_rule_cases_fire_and_meet_the_budget(tabs, tuples, table, feature, D, k):
    """the schedule of the exact GPU test: the rule fires, the budget binds somewhere, and no difference equals c"""
    ct, tup = tabs[table].ct, tuples[table]
    _, _, c = K.weather_rule(ct, feature, D, k)
    want, att = K.weather_rule_schedule(ct, feature, k, c, tup)
    assert want.any() and att.sum() > want.sum() and not want.all()
    h = LR.series(ct, feature)
    assert not ((h[:, k:] - h[:, :-k]).astype(np.float32) == c).any()


# ------------------------------------------------------------------ host packing
PACK_TABLES = ("permuted", "n8", "narrow")
PACK_DAYS = (4, 5, 8, 9)


@pytest.mark.parametrize("D", PACK_DAYS)
@pytest.mark.parametrize("table", PACK_TABLES)
def test_linear_weights_land_on_their_slots_and_lookahead_rows(tabs, table, D):
    ct = tabs[table].ct
    n_g = 2
    W = (np.arange(n_g * (ct.n_obs + D), dtype=np.float32).reshape(n_g, -1) + 1.0) / 8.0  # every value its own
    pol = dict(kind="linear", weight=W, bias=np.zeros(n_g, np.float32), group=np.array([0, 1, 1, 0]),
               lookahead=K.spec("heat_qi", D))
    a = P.check_linear_policy(pol, ct.n_obs, 4, ct.obs_slot, "cpu", ct.feature_names, (), ct.slot_of.get("alerts_2wks", -1))
    want = np.zeros((n_g, 32))
    for c in range(ct.n_obs):  # the slot layout restated: column c of the weight sits on slot obs_slot[c]
        want[:, ct.obs_slot[c]] = W[:, c]
    np.testing.assert_array_equal(a.weight_slots.numpy().astype(np.float64), want)
    look = np.zeros((n_g, P.LOOKAHEAD_PAD))
    look[:, :D] = W[:, ct.n_obs:]
    assert a.look_days == D and tuple(a.look_weight.shape) == (n_g, P.LOOKAHEAD_PAD)
    np.testing.assert_array_equal(a.look_weight.numpy().astype(np.float64), look)


@pytest.mark.parametrize("net", ["tanh7x13", "relu29_o2", "relu33"])
@pytest.mark.parametrize("D", PACK_DAYS)
@pytest.mark.parametrize("table", PACK_TABLES)
def test_mlp_first_layer_lands_on_its_slots_and_tail_rows(tabs, table, D, net):
    """pack_mlp against an fp64 restatement of the block: W1[32 slots][width] with observation column c on slot
    obs_slot[c], W1f[12][width] at the tail with lookahead column k on row k - 1, zero everywhere else; and pack ->
    unpack is the identity on the [G, out, n_obs + D] view (one output row: nothing is folded)."""
    ct = tabs[table].ct
    _, hidden, _, _ = M.MATRIX[net]
    rng = np.random.default_rng(D + len(net))
    L0 = LR.widen_net(M.net(ct, net, hidden, 1), D, seed=D)
    L = [(np.round(W * 64) / 64 + 1 / 128, np.round(b * 64) / 64) for W, b in L0]  # f32-exact, no first-layer weight zero
    packed, w, nl, n_g = P.pack_mlp(L, ct.obs_slot, ct.n_obs, D)
    assert (w, nl) == M.MATRIX[net][0] and packed.shape == (n_g, P.mlp_lookahead_stride(w, nl))
    W1 = L[0][0].astype(np.float64)
    head = np.zeros((n_g, 32, w))
    for c in range(ct.n_obs):
        head[:, ct.obs_slot[c], :hidden[0]] = W1[:, :, c]
    tail = np.zeros((n_g, P.LOOKAHEAD_PAD, w))
    for k in range(1, D + 1):
        tail[:, k - 1, :hidden[0]] = W1[:, :, ct.n_obs + k - 1]
    got = packed.numpy().astype(np.float64)
    np.testing.assert_array_equal(got[:, :32 * w].reshape(n_g, 32, w), head)
    np.testing.assert_array_equal(got[:, P.mlp_stride(w, nl):].reshape(n_g, P.LOOKAHEAD_PAD, w), tail)
    assert (tail[:, :D, :hidden[0]] != 0).all() and not tail[:, D:].any()
    # the block without the key: nothing before the tail moves
    plain = P.pack_mlp([(L[0][0][..., :ct.n_obs], L[0][1])] + L[1:], ct.obs_slot, ct.n_obs)[0]
    assert torch.equal(packed[:, :P.mlp_stride(w, nl)], plain)
    U = P.unpack_mlp_grad(packed, ct.obs_slot, ct.n_obs, hidden, 1, D)
    assert tuple(U[0][0].shape) == (n_g, hidden[0], ct.n_obs + D)
    for (Wl, bl), (dW, db) in zip(L, U):
        np.testing.assert_array_equal(dW.numpy(), Wl.astype(np.float32))
        np.testing.assert_array_equal(db.numpy(), bl.astype(np.float32))
    # a gradient-shaped block of its own: what unpack reads from the tail is row k - 1 for column n_obs + k - 1
    Pr = torch.as_tensor(rng.standard_normal(tuple(packed.shape)))
    dW1 = P.unpack_mlp_grad(Pr, ct.obs_slot, ct.n_obs, hidden, 1, D)[0][0].numpy()
    blk = Pr.numpy()
    for c in range(ct.n_obs):
        np.testing.assert_array_equal(dW1[:, :, c], blk[:, :32 * w].reshape(n_g, 32, w)[:, ct.obs_slot[c], :hidden[0]])
    for k in range(1, D + 1):
        np.testing.assert_array_equal(dW1[:, :, ct.n_obs + k - 1],
                                      blk[:, P.mlp_stride(w, nl):].reshape(n_g, P.LOOKAHEAD_PAD, w)[:, k - 1, :hidden[0]])


# ------------------------------------------------------------------ the feature check
@pytest.mark.parametrize("table", ["permuted", "n8"])
def test_check_lookahead_accepts_exactly_the_table_sourced_columns(tabs, table):
    ct = tabs[table].ct
    args = (ct.feature_names, ct.obs_slot, ct.n_obs, (), ct.slot_of.get("alerts_2wks", -1))
    assert set(K.RUN_TIME_COLUMNS) <= set(ct.feature_names) and "alerts_2wks" in ct.feature_names
    assert ct.obs_slot[ct.feature_names.index("alert_2wks")] == 27
    for name in ct.feature_names:
        pol = {"lookahead": K.spec(name, 3)}
        if name in K.RUN_TIME_COLUMNS:
            with pytest.raises(ValueError, match="table-sourced"):
                P.check_lookahead(pol, "test", *args)
        else:
            assert P.check_lookahead(pol, "test", *args) == (name, 3)
    with pytest.raises(ValueError, match="no observation column"):
        P.check_lookahead({"lookahead": K.spec("no_such_column", 3)}, "test", *args)
