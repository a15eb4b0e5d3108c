"""The cases of tests/test_lookahead_layouts_gpu.py, shared with tests/test_lookahead_layouts_cpu.py, which walks every
rollout case on the host oracle alone: policy["lookahead"] on the observation layouts of tests/obs_layouts.py (columns on
slots that are not their index, n_obs of 29, 28, 8 and 5, the ragged variants) and on the slot-27 tables of
tests/table_edges.py, with lookahead features other than heat_qi and D on both sides of every k-step of four (4, 5, 8,
9). Batch size, groups and the policies are those of tests/lookahead_cases.py; the reset settings and the policy seeds
are the tables' own. Nothing here touches the GPU or the library's kernels."""
import numpy as np

import lookahead_cases as C
import lookahead_restatement as LR
import obs_layouts as L
import policy_gradient_mlp_cases as M
import table_edges as E

N, G, GID0 = C.N, C.G, C.GID0  # 193 envs (no multiple of 64), three interleaved groups
LAYOUT_TABLES = L.LAYOUTS + L.RAGGED
SLOT27_TABLES = ("slot27", "ragged27")
RUN_TIME_COLUMNS = ("alert_lag1", "alert_streak", "remaining_budget", "alert_2wks")  # slots 24..27: never table-sourced

# (table, feature, D, sample)
LINEAR_CASES = [("permuted", "heat_qi", 4, False), ("permuted", "weekend", 5, True), ("n28", "heat_qi", 8, True),
                ("n8", "hi_max", 2, False), ("n8", "alerts_2wks", 3, True), ("n8", "heat_qi", 9, True),
                ("narrow", "heat_qi", 5, False), ("permuted_ragged", "heat_qi", 10, True),
                ("n8_ragged", "hi_max", 4, False), ("slot27", "heat_qi", 4, False), ("ragged27", "heat_qi", 5, True)]
# (table, feature, D, sample, net of policy_gradient_mlp_cases.MATRIX): all six <WIDTH, LAYERS>, every D of {2, 4, 5, 8, 9}
MLP_CASES = [("permuted", "heat_qi", 5, False, "tanh7x13"), ("n28", "weekend", 4, True, "tanh17"),
             ("n8", "hi_max", 9, False, "relu33"), ("n8", "alerts_2wks", 2, True, "tanh29x9"),
             ("narrow", "heat_qi", 8, True, "relu40x64"), ("n8_ragged", "heat_qi", 5, True, "tanh1_o2"),
             ("ragged27", "heat_qi", 9, False, "tanh64x33_o2"), ("narrow", "heat_qi", 4, True, "relu29_o2")]
# (kind, table, lookahead feature, D, gate feature, net): the gate reads another column than the lookahead does
GATE_CASES = [("linear", "permuted_ragged", "heat_qi", 8, "hi_max", None),
              ("mlp", "permuted_ragged", "heat_qi", 9, "heat_qi_3d", "tanh17")]
GATE_QUANTILE = 0.4  # the gate's threshold: this quantile of its column over every episode's days
# (table, feature, D): sampled linear policies whose group means must hold no near-tie env at all
GRADIENT_CASES = [("permuted_ragged", "heat_qi", 5), ("n8", "hi_max", 4), ("narrow", "heat_qi", 9)]
IMITATION_CASES = [("n8", "hi_max", 4), ("permuted", "weekend", 8)]
IMITATION_P, IMITATION_SEED = 0.35, 21  # the fixed Bernoulli schedule of the imitation cases
# (table, feature, D, k): observation weights 0, weight 1 on lookahead input k, bias -midpoint_threshold
WEATHER_RULE_CASES = [("permuted", "heat_qi", 5, 5), ("n8", "hi_max", 4, 4), ("n8", "heat_qi", 8, 5),
                      ("n8_ragged", "hi_max", 9, 9)]
# the scale of the appended lookahead columns (lookahead_restatement.widen_*: 0.5) per feature, where 0.5 lets the
# lookahead inputs decide too little (tests/test_lookahead_layouts_cpu.py: one env in ten must depend on them)
LOOK_SCALE = {}
# weight seeds moved off lookahead_cases.linear's 3 where a case met the near-tie cap: (table, feature, D) -> seed
WEIGHT_SEEDS = {}


def make_tables():
    """name -> table_edges.Table: the six layout tables (T = 40) and the two slot-27 tables (T = 60)"""
    tabs = dict(L.make_layouts())
    edges = E.make_tables()
    tabs.update({k: edges[k] for k in SLOT27_TABLES})
    return tabs


def reset_cfg(name):
    return L.RESET[name] if name in L.RESET else E.RESET[name]


def host_tuples(tb):
    """the episode tuples env.reset(seed, options) draws for the N envs of the GPU tests"""
    return E.host_tuples(tb, N, reset_cfg(tb.name))


def spec(feature, D):
    return {"feature": feature, "days": D}


def policy_seed(name):
    return L.policy_seed(name)


def uniform(name):
    """u of (seed, global env id, episode 0, day) under the table's policy seed"""
    return LR.policy_uniform(policy_seed(name), GID0, {"episode_no": np.zeros(N, np.int64)})


def linear(tb, feature, D, sample=False, **kw):
    """lookahead_cases.linear on the table's own columns, feature and policy seed"""
    ct = tb.ct
    seed = WEIGHT_SEEDS.get((tb.name, feature, D), 3)
    W, b = E.linear_params(ct, seed=seed)
    W = LR.widen_linear(ct, W[:G], D, seed=seed + D, scale=LOOK_SCALE.get(feature, 0.5))
    return dict(kind="linear", weight=W, bias=b[:G], group=C.groups(), sample=sample, seed=policy_seed(tb.name),
                lookahead=spec(feature, D), **kw)


def mlp(tb, feature, name, D, sample=False, **kw):
    """lookahead_cases.mlp: the net `name` of the instantiation matrix at the table's n_obs, the first layer D wider"""
    _, hidden, act, n_out = M.MATRIX[name]
    layers = [(W[:G], b[:G]) for W, b in LR.widen_net(M.net(tb.ct, name, hidden, n_out), D, seed=D + len(name),
                                                      scale=LOOK_SCALE.get(feature, 0.5))]
    return dict(kind="mlp", layers=layers, activation=act, group=C.groups(), sample=sample, seed=policy_seed(tb.name),
                lookahead=spec(feature, D), **kw)


def without(pol, ct):
    """the policy without the key and without its lookahead columns"""
    p = {k: v for k, v in pol.items() if k != "lookahead"}
    if p["kind"] == "linear":
        p["weight"] = pol["weight"][:, :ct.n_obs]
    else:
        p["layers"] = [(pol["layers"][0][0][..., :ct.n_obs], pol["layers"][0][1])] + list(pol["layers"][1:])
    return p


def zeroed(pol, ct):
    """the policy with its lookahead columns set to zero"""
    p = dict(pol)
    if p["kind"] == "linear":
        p["weight"] = pol["weight"].copy()
        p["weight"][:, ct.n_obs:] = 0
    else:
        W1 = pol["layers"][0][0].copy()
        W1[..., ct.n_obs:] = 0
        p["layers"] = [(W1, pol["layers"][0][1])] + list(pol["layers"][1:])
    return p


def gate_threshold(ct, feature):
    """f32: GATE_QUANTILE of the gate's column over the days of every episode of the table (rows past an episode's
    end are padding)"""
    slot = ct.obs_slot[ct.feature_names.index(feature)]
    x = np.asarray(ct.X)[:, :, slot].astype(np.float64)
    live = np.arange(ct.T)[:, None] < np.asarray(ct.n_days).reshape(-1)[None, :]
    return float(np.float32(np.quantile(x[live], GATE_QUANTILE)))


def imitation_schedule(ct):
    return np.random.default_rng(IMITATION_SEED).random((N, ct.T)) < IMITATION_P


def weather_rule(ct, feature, D, k):
    """the policy of the exact test: (weight [G, n_obs + D], bias [G], c)"""
    c = LR.midpoint_threshold(ct, feature, k)
    W = np.zeros((G, ct.n_obs + D), np.float32)
    W[:, ct.n_obs + k - 1] = 1.0
    return W, np.full(G, -c, np.float32), c


def weather_rule_schedule(ct, feature, k, c, st):
    """(alert_days, attempt_days) bool [N, T] the table and the budget rule give for `f_k > c` from a reset state
    (county_w, year_i, n_days, budget): every value is an f32 of the table, no logit is evaluated"""
    h = LR.series(ct, feature)
    row = np.asarray(st["county_w"], np.int64) * ct.Y + np.asarray(st["year_i"], np.int64)
    n = len(row)
    want, att = np.zeros((n, ct.T), bool), np.zeros((n, ct.T), bool)
    for e in range(n):
        used, nd = 0, int(st["n_days"][e])
        for t in range(nd):
            r = max(t - 1, 0)
            f = np.float32(h[row[e], r + k] - h[row[e], r]) if r + k < nd else np.float32(0)
            att[e, t] = f > c
            want[e, t] = att[e, t] and used < st["budget"][e]
            used += want[e, t]
    return want, att
