"""The table edges every day-loop copy is held to (tests/test_table_edges_gpu.py, tests/test_table_edges_cpu.py): three
synthetic tables, the batches drawn on them, the policies, and the fp64 `a = policy(obs); step(a)` loop on the vector
oracle that records what rollout(record=True) records. Nothing here touches the GPU or the library.

  ragged    episodes of 20..153 days over four years, one pair at the full T, and the shortest episodes there are: 1, 2
            and 3 days (tables.compile_from_synth accepts all three; it refuses none, a length of 0 is a hole)
  slot27    uniform 60-day episodes; a third of the coefficient columns with a coefficient on slot 27 (the agent's
            14-day alert count, `alert_2wks`) ~ N(0, 0.05), a third with the large heat_qi / bias pair (+30 / -15),
            the rest untouched -- as tests/test_env_gpu.py::test_matrix_core_rollout_exact_path_and_slot27_rows
  ragged27  both: slot27's coefficients on episodes of 15..60 days, and of 1, 2 and 3

The oracle (like the reference's weight files) has no slot-27 key: on the slot-27 tables its rewards are right only for
envs whose coefficient column has none (`known`); its observations, decisions and integer state do not depend on the
reward and are right for every env."""
from __future__ import annotations

import copy

import numpy as np

from oracle import heatalert_oracle as O
from posterior_restatement import posterior_returns_fp64
from weather2alert_amd import synth, tables

GID0 = 300
SHORTEST = (1, 2, 3)


class Table:
    def __init__(self, name, sd, nd=None, slot27=False):
        self.name, self.slot27, self.ragged = name, slot27, nd is not None
        S = len(sd.fips_list)
        self.big, self.a2w = np.zeros(S, bool), np.zeros(S, bool)
        if nd is not None:
            sd.meta["n_days_per_episode"] = nd
        sd_oracle = sd
        if slot27:
            self.big, self.a2w = np.arange(S) % 3 == 0, np.arange(S) % 3 == 1
            big = self.big.astype(np.float32)[None, None, :]
            rng = np.random.default_rng(3)
            w = sd.weights
            w["baseline_heat_qi"] = w["baseline_heat_qi"] + 30.0 * big
            w["baseline_bias"] = w["baseline_bias"] - 15.0 * big
            w["effectiveness_heat_qi"] = w["effectiveness_heat_qi"] + 24.0 * big
            w["effectiveness_bias"] = w["effectiveness_bias"] - 12.0 * big
            sd_oracle = copy.copy(sd)
            sd_oracle.weights = dict(w)  # the oracle's weights: without the key no reference weights file has
            for head in ("baseline", "effectiveness"):
                w[f"{head}_alert_2wks"] = (rng.normal(0, 0.05, w["baseline_bias"].shape) * self.a2w[None, None, :]).astype(np.float32)
        self.sd, self.ct = sd, tables.compile_from_synth(sd)
        self.ref = O.RefData.from_synth(sd_oracle)

    def oracle(self, reward_mode="sampled"):
        return O.VectorOracle(self.ref, self.sd.fips_weather, self.sd.years, reward_mode=reward_mode)


def _lengths(sd, lo, hi, seed):
    S_w, Y, T = sd.alert.shape
    nd = np.random.default_rng(seed).integers(lo, hi + 1, size=(S_w, Y))
    nd[0, 0] = T
    for k, d in enumerate(SHORTEST):
        nd[1 + k, k % Y] = d
    return nd


def make_tables():
    """{"ragged", "slot27", "ragged27"} -> Table"""
    kw = dict(n_fips=30, n_samples=6, extra_confounder_fips=3)
    r = synth.make_synth("linear", years=[2006, 2007, 2008, 2009], seed=17, **kw)
    s = synth.make_synth("linear", years=[2006, 2007], n_days=60, seed=29, **kw)
    b = synth.make_synth("linear", years=[2006, 2007, 2008, 2009], n_days=60, seed=31, **kw)
    return {"ragged": Table("ragged", r, _lengths(r, 20, 153, 1)), "slot27": Table("slot27", s, slot27=True),
            "ragged27": Table("ragged27", b, _lengths(b, 15, 60, 2), slot27=True)}


# ------------------------------------------------------------------ batches
# reset options of each table's batch: budgets drawn in [0, default] (zeros included, most above the shortest episodes)
RESET = {"ragged": dict(seed=5, opts={"sample_budget": True, "sample_budget_type": "less_than"}),
         "slot27": dict(seed=6, opts={"budget": 12}),
         "ragged27": dict(seed=7, opts={"sample_budget": True, "sample_budget_type": "less_than"})}
N_ENVS = {"ragged": 2000 + 37, "slot27": 1500 + 11, "ragged27": 2500 + 29}  # no multiples of 64 or 256


def host_tuples(tb: Table, n: int, cfg=None):
    """The episode tuples env.reset(seed=RESET[..]["seed"], options=RESET[..]["opts"]) draws on a fresh env with
    env_gid0=GID0 and similar_climate_counties=True (the oracle's restatement of the device RNG). `cfg`: the reset
    settings of a table that is not one of the three above (tests/obs_layouts.py)."""
    ct, cfg = tb.ct, (RESET[tb.name] if cfg is None else cfg)
    mode = 1 if cfg["opts"].get("sample_budget") else 0
    bkw = int(cfg["opts"].get("budget", -1))
    rows = [O.devrng_reset_tuple(cfg["seed"], GID0 + i, 0, ct.S, ct.Y, ct.n_samples, ct.fips_to_weather, ct.sim_ptr,
                                 ct.sim_cnt, True, lambda cw, yi: int(ct.B0[cw * ct.Y + yi]), -1, bkw, mode)
            for i in range(n)]
    cw, cc, yi, sm, b = (np.array(c, np.int64) for c in zip(*rows))
    return dict(county_w=cw, coef_col=cc, year_i=yi, sample=sm, budget=b, n_days=ct.n_days[cw * ct.Y + yi].astype(np.int64))


def oracle_reset(V, tup):
    V.reset(tup["county_w"], tup["year_i"], tup["coef_col"], tup["sample"], tup["budget"])
    V._finished = np.zeros(len(tup["budget"]), bool)


def lengths_per_wave(n_days):
    """mean number of distinct episode lengths among 64 consecutive env ids"""
    return float(np.mean([len(np.unique(n_days[i:i + 64])) for i in range(0, len(n_days), 64)]))


# ------------------------------------------------------------------ policies
G = 5


def groups(n):
    """interleaved: most waves hold all five groups"""
    return (np.arange(n) * 3 + np.arange(n) // 7) % G


def _col_scale(ct):
    s = np.ones(ct.n_obs)
    s[ct.feature_names.index("remaining_budget")] = 0.1
    return s


def linear_params(ct, seed=3, scale=0.4):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((G, ct.n_obs)) * scale * _col_scale(ct)).astype(np.float32)
    return W, (rng.standard_normal(G) * 0.5).astype(np.float32)


def net(ct, hidden, n_out, seed):
    rng = np.random.default_rng(seed)
    dims = [ct.n_obs] + list(hidden) + [n_out]
    layers = []
    for i in range(len(dims) - 1):
        W = rng.standard_normal((G, dims[i + 1], dims[i])) * (1.5 / np.sqrt(dims[i]))
        if i == 0:
            W *= _col_scale(ct)[None, None, :]
        layers.append((W.astype(np.float32), (rng.standard_normal((G, dims[i + 1])) * 0.5).astype(np.float32)))
    return layers


def mlp64(layers, activation, obs, g):
    """fp64 logits of the f32 parameters on f32 rows and each one's near-tie scale |b_out| + sum_h |w_out,h h_h| (two
    outputs folded into row1 - row0 and rounded to f32 once, as the host does)."""
    act = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0.0))
    h = obs.astype(np.float64)
    for W, b in layers[:-1]:
        nxt = np.empty((len(h), W.shape[1]))
        for k in range(W.shape[0]):
            nxt[g == k] = act(h[g == k] @ W[k].astype(np.float64).T + b[k].astype(np.float64))
        h = nxt
    Wo, bo = layers[-1]
    Wo, bo = Wo.astype(np.float64), bo.astype(np.float64)
    if Wo.shape[1] == 2:
        Wo, bo = Wo[:, 1:] - Wo[:, :1], bo[:, 1:] - bo[:, :1]
    Wo, bo = Wo.astype(np.float32).astype(np.float64)[:, 0], bo.astype(np.float32).astype(np.float64)[:, 0]
    prod = Wo[g] * h
    return prod.sum(axis=1) + bo[g], np.abs(prod).sum(axis=1) + np.abs(bo[g])


# name -> (kind, sample): the linear policy, a one-layer ReLU net with one output row, a [64, 64] tanh net with two
POLICIES = {"linear": ("linear", False), "linear_sampled": ("linear", True), "mlp16": ("mlp16", False),
            "mlp16_sampled": ("mlp16", True), "mlp64x64": ("mlp64x64", False), "mlp64x64_sampled": ("mlp64x64", True)}
POLICY_SEED = 11


def make_policy(ct, name, g):
    """(policy dict for rollout(), fp64 logit function obs -> (z, near-tie scale), near-tie bounds (rel, sampled)):
    the bounds are those of tests/test_linear_policy_gpu.py (1e-9, 1e-6) and tests/test_mlp_policy_gpu.py (1e-5, 1e-5)"""
    kind, sample = POLICIES[name]
    if kind == "linear":
        W, b = linear_params(ct)
        W64, b64 = W.astype(np.float64)[g], b.astype(np.float64)[g]

        def fn(obs):
            prod = obs.astype(np.float64) * W64
            return prod.sum(axis=1) + b64, np.abs(prod).sum(axis=1) + np.abs(b64)
        return dict(kind="linear", weight=W, bias=b, group=g, sample=sample, seed=POLICY_SEED), fn, (1e-9, 1e-6)
    hidden, act, n_out = ((16,), "relu", 1) if kind == "mlp16" else ((64, 64), "tanh", 2)
    layers = net(ct, hidden, n_out, seed=len(hidden) * 10 + hidden[0])
    return (dict(kind="mlp", layers=layers, activation=act, group=g, sample=sample, seed=POLICY_SEED),
            (lambda obs: mlp64(layers, act, obs, g)), (1e-5, 1e-5))


def policy_uniform(n):
    """the sampled policies' uniform of (env, episode 0, day t)"""
    return lambda t: O.devrng_policy_uniform_vec(POLICY_SEED, GID0 + np.arange(n), np.zeros(n, np.int64), t)


# ------------------------------------------------------------------ the oracle's loop
_FROZEN = ("t", "used", "streak", "hist", "last_actual", "at_budget", "obs")


def oracle_step(V, act):
    """V.step(act) that leaves envs already in V._finished untouched (the oracle itself would go on shifting their
    history); marks envs whose terminal step this was. Returns (reward, done, actual, live)."""
    live = ~V._finished
    keep = {k: getattr(V, k).copy() for k in _FROZEN}
    _, r, done, actual = V.step(np.where(live, act, 0))
    for k, v in keep.items():
        cur = getattr(V, k)
        cur[~live] = v[~live]
    V._finished = V._finished | (live & done)
    return r, done, actual, live


def oracle_state(V):
    return dict(t=V.t, used=V.used, streak=V.streak, last_actual=V.last_actual, at_budget=V.at_budget.astype(np.int64),
                hist14=(V.hist * (1 << np.arange(13, -1, -1))[None, :]).sum(axis=1), finished=V._finished.astype(np.int64))


def oracle_record(V, logit_fn, S, ties, uniform=None, T=None):
    """`a = policy(V.obs); V.step(a)` for S days, recorded like rollout(record=True): numpy arrays [S(+1), n, ...], the
    fp64 logits, and what rollout() itself returns (ret, alerts, over, alert / attempt bitmaps by episode day) -- plus a
    per-env near-tie flag (an env with a tie anywhere is left out: after a differing decision its trajectory
    legitimately diverges)."""
    n, n_obs = V.obs.shape
    T = S if T is None else T
    R = dict(obs=np.zeros((S + 1, n, n_obs), np.float32), action=np.zeros((S, n), np.uint8), logit=np.zeros((S, n)),
             mag=np.zeros((S, n)), reward=np.zeros((S, n)), valid=np.zeros((S, n), bool),
             terminated=np.zeros((S, n), bool), alert=np.zeros((S, n), bool), tie=np.zeros(n, bool), t0=V.t.copy(),
             ret=np.zeros(n), alerts=np.zeros(n, np.int64), over=np.zeros(n, np.int64), days=np.zeros((n, T), bool),
             att=np.zeros((n, T), bool))
    rows = np.arange(n)
    for s in range(S):
        live = ~V._finished
        R["obs"][s] = V.obs.astype(np.float32)
        if not live.any():
            continue
        z, mag = logit_fn(R["obs"][s])
        if uniform is None:
            act = z > 0
            R["tie"] |= live & (np.abs(z) <= ties[0] * mag)
        else:
            sg = 1.0 / (1.0 + np.exp(-z))
            u = uniform(V.t).astype(np.float64)
            act = u < sg
            R["tie"] |= live & (np.abs(sg - u) <= ties[1])
        act = (act & live).astype(np.int64)
        tday, atb = V.t.copy(), V.used == V.budget
        r, done, actual, _ = oracle_step(V, act)
        R["action"][s] = act
        R["logit"][s], R["mag"][s], R["reward"][s] = z, mag, np.where(live, r, 0.0)
        R["valid"][s], R["terminated"][s], R["alert"][s] = live, live & done, live & (actual == 1)
        R["ret"] += np.where(live, r, 0.0)
        R["alerts"] += np.where(live, actual, 0)
        R["over"] += np.where(live & (act == 1) & atb, 1, 0)
        R["days"][rows[live & (actual == 1)], tday[live & (actual == 1)]] = True
        R["att"][rows[live & (act == 1)], tday[live & (act == 1)]] = True
    R["obs"][S] = V.obs.astype(np.float32)
    return R


# ------------------------------------------------------------------ reward_mode="posterior_mean"
PR_KEYS = ("t", "used", "streak", "hist14", "budget", "n_days", "county_w", "year_i", "coef_col", "finished")


def start_state(tup):
    """the state() of a batch right after the reset that drew `tup` (host_tuples), as the restatements take it"""
    z = np.zeros(len(tup["budget"]), np.int64)
    return dict(t=z, used=z, streak=z, hist14=z, finished=z,
                **{k: tup[k] for k in ("budget", "n_days", "county_w", "year_i", "coef_col")})


def pm_rewards_fp64(ct, start, alert_days, n_steps):
    """The posterior-mean reward in fp64 with every slot, slot 27 included: the mean over the draw axis of the
    restatement's per-day rewards (tests/posterior_restatement.py). start: a state() dict (PR_KEYS are read);
    alert_days bool [N, >= T]. Returns ([n_steps, N] rewards, NaN where the env did not step; [N] summed return)."""
    st = {k: np.asarray(start[k]) for k in PR_KEYS}
    ret, days = posterior_returns_fp64(ct.X, ct.W, ct.n_samples, ct.Y, st, np.asarray(alert_days), n_steps, per_day=True)
    return days.mean(axis=2).T, ret.mean(axis=1)


def pi8_flagged_columns(ct, max_budget):
    """Host restatement of which coefficient columns the int8 posterior-mean kernels send down their exact fp64 path
    (k_pi8_slot_max, k_pi8_scales and the flag test of k_pi8_wq): 2^ex_k is the power of two above the largest |x_k| of
    slot k -- over the whole feature table for the table-sourced slots, from the run-time slots' ranges for a batch
    whose largest budget is `max_budget` (lag 1, streak min(T, B), remaining budget B, 14-day count min(14, B)) -- and
    a column is flagged when frexp(max_k |w_k| 2^ex_k) of any of its coefficient rows has an exponent above 4. Reads
    nothing from the device; bool [S]."""
    xmax = np.abs(np.asarray(ct.X, np.float64)).reshape(-1, 32).max(axis=0)
    b = float(max_budget)
    xmax[24:28] = 1.0, min(float(ct.T), b), b, min(14.0, b)
    ex = np.where(xmax > 0, np.frexp(xmax)[1], 0)
    W = np.abs(np.asarray(ct.W, np.float64)).reshape(-1, ct.n_samples * 2, 32)  # [S, rows of the column, 32]
    m = (W * np.ldexp(1.0, ex)[None, None, :]).max(axis=2)
    ew = np.where(m > 0, np.frexp(m)[1], 0)
    return (ew > 4).any(axis=1)


def builtin_policies(ct):
    """kind -> the policy dict rollout() takes (oracle_policy() makes it the one O.oracle_rollout takes). The kinds
    decide on table-sourced columns, the remaining budget and the device RNG, all of which the oracle restates
    exactly: no env is a near-tie."""
    table = (np.random.default_rng(0).random((ct.T, 5)) < 0.3).astype(np.uint8)
    return {"bernoulli": dict(kind="bernoulli", p=0.3, seed=POLICY_SEED),
            "threshold": dict(kind="threshold", feature="heat_qi", threshold=0.8, require_budget=True),
            "table": dict(kind="table", table=table), "always": dict(kind="always")}


def oracle_policy(ct, pol):
    return dict(pol, col=ct.columns.index("heat_qi"))


class PolicyStream:
    """O.oracle_rollout's seed_stream for the bernoulli kind: the device RNG's uniform of (env, episode_no, day)"""

    def __init__(self, n, episode_no=None, seed=POLICY_SEED):
        self.seed, self.gid = seed, GID0 + np.arange(n)
        self.episode_no = np.zeros(n, np.int64) if episode_no is None else np.asarray(episode_no, np.int64)

    def vec(self, t):
        return O.devrng_policy_uniform_vec(self.seed, self.gid, self.episode_no, t)


def oracle_builtin_rollout(V, opol, n_steps, stream=None):
    """O.oracle_rollout(V, opol, n_steps, stream) and, beside its (ret, alerts, over, alert days), the attempt days:
    the actions the loop hands to V.step, by episode day, for the envs still running."""
    n, T = len(V.t), V.X.shape[2]
    att = np.zeros((n, T), bool)
    step = V.step

    def spy(act):
        sel = ~V._finished & (np.asarray(act) == 1)
        att[np.arange(n)[sel], V.t[sel]] = True
        return step(act)

    V.step = spy
    try:
        ret, alerts, over, days = O.oracle_rollout(V, opol, n_steps, stream)
    finally:
        del V.step
    return dict(ret=ret, alerts=alerts, over=over, days=days, att=att)


def pm_step_reference(tb, n, seed=12, p=0.3):
    """step() for ct.T days with random actions (zeroed once an env is finished) on the posterior-mean oracle, and the
    fp64 reference of the same days: dict(actions int32 [T, n], live bool [T, n], done bool [T, n], oracle f64 [T, n]
    (right on the `known` envs), alert_days bool [n, T], reward f64 [T, n] (NaN where the env did not step), ret [n],
    known [n], tup)."""
    ct = tb.ct
    tup = host_tuples(tb, n)
    V = tb.oracle("posterior_mean")
    oracle_reset(V, tup)
    rng = np.random.default_rng(seed)
    T = ct.T
    R = dict(actions=np.zeros((T, n), np.int32), live=np.zeros((T, n), bool), done=np.zeros((T, n), bool),
             oracle=np.zeros((T, n)), alert_days=np.zeros((n, T), bool), tup=tup, known=~tb.a2w[tup["coef_col"]])
    rows = np.arange(n)
    for s in range(T):
        act = np.where(V._finished, 0, rng.random(n) < p).astype(np.int32)
        tday = V.t.copy()
        r, done, actual, live = oracle_step(V, act)
        R["actions"][s], R["live"][s], R["done"][s], R["oracle"][s] = act, live, live & done, np.where(live, r, 0.0)
        R["alert_days"][rows[live & (actual == 1)], tday[live & (actual == 1)]] = True
    assert V._finished.all()
    R["reward"], R["ret"] = pm_rewards_fp64(ct, start_state(tup), R["alert_days"], T)
    R["state"] = oracle_state(V)
    return R
