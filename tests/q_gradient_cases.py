"""The cases of tests/test_q_gradient_gpu.py, shared with tests/test_q_gradient_cpu.py: which net, table, prefix,
schedule and estimator settings every comparison runs, and everything about a case that is decided on the host -- the
nets, the groups, the days before the call, the schedule. The CPU file replays every case with the NumPy oracle (the
device RNG's reset restated by tests/table_edges.py) and holds the restatement's own ambiguity shares under the cap;
the GPU file runs the kernels against a twin stepped through step(). Nothing here touches the GPU or the library."""
import numpy as np

import table_edges as E
from oracle import heatalert_oracle as O
from weather2alert_amd import synth, tables

N, G = 300, 4  # four full waves and a partial one; groups 0, 1 and 3 hold envs, group 2 is empty
GROUP_SIZE = 1000  # the large cases: groups of consecutive env ids
N_LARGE = (1 << 17) + 200  # 131 272 envs = 2 052 tiles: 3 per wave of the second pass


class _Synth:
    """a synthetic table in the form tests/table_edges.py gives its own (ct, the oracle's data)"""
    def __init__(self, name, **kw):
        self.name = name
        self.sd = synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=6, extra_confounder_fips=3, **kw)
        self.ct = tables.compile_from_synth(self.sd)
        self.ref = O.RefData.from_synth(self.sd)

    def oracle(self):
        return O.VectorOracle(self.ref, self.sd.fips_weather, self.sd.years)


RESET = {"synth": dict(seed=5, opts={"budget": 10}), "short": dict(seed=79, opts={"budget": 4}),
         "ragged": E.RESET["ragged"]}


def make_tables():
    """name -> table: the 153-day synthetic table of the other gradient tests, a 12-day one for the large batches, and
    the ragged table of tests/table_edges.py"""
    return {"synth": _Synth("synth", seed=17), "short": _Synth("short", n_days=12, seed=23),
            "ragged": E.make_tables()["ragged"]}


# (hidden widths, the net's seed). The six shapes the feature was specified with reach five of the six <WIDTH, LAYERS>
# instantiations -- (24, 40) pads to width 64, like (64, 64) -- so (24, 20) is here for <32, 2>; every net but the last has
# padded units. A seed is changed here when a net's ambiguity share (near ties and ReLU kinks) exceeds the cap on a case
# below.
NETS = {"h7": ((7,), 71), "h24": ((24,), 241), "h40": ((40,), 401), "h7x13": ((7, 13), 713), "h24x20": ((24, 20), 2420),
        "h24x40": ((24, 40), 2440), "h64x64": ((64, 64), 6464)}
INSTANTIATION = {"h7": (16, 1), "h24": (32, 1), "h40": (64, 1), "h7x13": (16, 2), "h24x20": (32, 2), "h24x40": (64, 2),
                 "h64x64": (64, 2)}

DEFAULT = dict(table="synth", n=N, prefix=9, n_steps=None, bootstrap=False, target=True, double=False, loss="huber",
               huber_delta=2.0, gamma=0.99, rb=False, sched="random", weights=True, grouped=True, order=False)
# name -> what differs from DEFAULT. target: a distinct target net (False: target_net=None)
CASES = {
    "h7_tanh": dict(net="h7", act="tanh"),
    "h7_relu_double_gamma09": dict(net="h7", act="relu", double=True, gamma=0.9, huber_delta=4.0),
    "h24_relu_own_target_double_squared": dict(net="h24", act="relu", target=False, double=True, loss="squared", gamma=1.0,
                                               prefix=0),
    "h40_tanh_n3_bootstrap_double": dict(net="h40", act="tanh", double=True, gamma=0.9, n_steps=3, bootstrap=True),
    "h7x13_relu_order_double": dict(net="h7x13", act="relu", double=True, order=True, huber_delta=10.0),
    "h7x13_tanh_n1": dict(net="h7x13", act="tanh", target=False, n_steps=1),
    "h24x20_tanh_double": dict(net="h24x20", act="tanh", double=True, gamma=0.9),
    "h24x20_relu_at_budget_masked_order": dict(net="h24x20", act="relu", rb=True, sched="sampled", order=True,
                                               huber_delta=10.0),
    "h24x40_tanh_at_budget_masked_double": dict(net="h24x40", act="tanh", double=True, rb=True, sched="sampled"),
    "h24x40_relu_at_budget_masked_max": dict(net="h24x40", act="relu", rb=True, sched="sampled", huber_delta=10.0),
    "h64x64_relu_n3_squared": dict(net="h64x64", act="relu", loss="squared", gamma=0.9, n_steps=3),
    "h64x64_tanh_n1_bootstrap": dict(net="h64x64", act="tanh", n_steps=1, bootstrap=True, target=False),
    "h40_relu_ragged_finished_on_entry": dict(net="h40", act="relu", table="ragged", prefix=25, double=True, huber_delta=10.0),
    "h24_tanh_one_group_no_weights": dict(net="h24", act="tanh", grouped=False, weights=False, prefix=0, gamma=1.0),
}
# the six instantiations at 3 tiles per wave (<32, 2> under both activations, the others with the activation their 1-tile
# cases give least): 131 272 envs on the 12-day table, groups of
# 1 000 consecutive env ids, the groups of CHECKED rebuilt as small batches with the same global env ids
LARGE = {"h7_relu": dict(net="h7", act="relu", double=True, huber_delta=4.0), "h24_tanh": dict(net="h24", act="tanh", loss="squared"),
         "h40_relu": dict(net="h40", act="relu", target=False, huber_delta=4.0), "h7x13_tanh": dict(net="h7x13", act="tanh", double=True),
         "h24x20_relu": dict(net="h24x20", act="relu", rb=True, double=True, huber_delta=4.0),
         "h24x20_tanh": dict(net="h24x20", act="tanh"),
         "h24x40_relu": dict(net="h24x40", act="relu", rb=True, huber_delta=4.0), "h64x64_tanh": dict(net="h64x64", act="tanh", gamma=0.9)}
LARGE_DEFAULT = dict(DEFAULT, table="short", n=N_LARGE, prefix=2, sched="dense", huber_delta=2.0)
CHECKED = (2, 70, (N_LARGE - 1) // GROUP_SIZE)  # the last group has 272 envs


def case(name):
    return dict(DEFAULT, **CASES[name]) if name in CASES else dict(LARGE_DEFAULT, **LARGE[name])


def groups(n):
    return np.array([0, 1, 3])[np.arange(n) % 3]


def qnet(ct, name, G_, seed_shift=0):
    """[(W [G_, out, in], b [G_, out]), ...] with a two-row output (tests/table_edges.py: net, which draws E.G blocks)"""
    hidden, seed = NETS[name]
    layers = E.net(ct, hidden, 2, seed + seed_shift)
    reps = (G_ + E.G - 1) // E.G
    return [(np.concatenate([W] * reps)[:G_].copy(), np.concatenate([b] * reps)[:G_].copy()) for W, b in layers]


def nets(ct, c, G_):
    """(online layers, target layers or None): the target net is another draw of the same shape"""
    return qnet(ct, c["net"], G_), (qnet(ct, c["net"], G_, seed_shift=1) if c["target"] else None)


def scaled(layers, G_, seed):
    """group 0's block scaled down per group (the large cases' G_ = 132 groups)"""
    rng = np.random.default_rng(seed)
    return [(np.repeat(W[:1], G_, axis=0) * rng.uniform(0.5, 1.0, (G_, 1, 1)).astype(np.float32),
             np.repeat(b[:1], G_, axis=0) * rng.uniform(0.5, 1.0, (G_, 1)).astype(np.float32)) for W, b in layers]


def weights(n):
    w = np.random.default_rng(8).standard_normal(n).astype(np.float32)  # negative values
    w[::5] = 0.0
    return w


def prefix_actions(n, day, gid0=E.GID0):
    """the attempts of the days before the call: fixed per (global env id, day), so that a small batch rebuilt with the
    same global env ids walks the same prefix"""
    gid = gid0 + np.arange(n, dtype=np.uint64)
    h = (gid * np.uint64(2654435761) + np.uint64(day + 1) * np.uint64(40503)) % np.uint64(1000)
    return (h < np.uint64(400)).astype(np.int32)


def host_schedule(kind, n, T, gid0=E.GID0):
    """bool [n, T] by day of the episode, a function of the global env id: "random" 35 % of the days, "dense" 60 %"""
    gid = gid0 + np.arange(n, dtype=np.uint64)[:, None]
    h = (gid * np.uint64(2246822519) + np.arange(T, dtype=np.uint64)[None, :] * np.uint64(3266489917)) % np.uint64(1000)
    return h < np.uint64(350 if kind == "random" else 600)


def tuples(ct, cfg, n, gid0=E.GID0):
    """tests/table_edges.py: host_tuples for any table and first global env id"""
    mode = 1 if cfg["opts"].get("sample_budget") else 0
    bkw = int(cfg["opts"].get("budget", -1))
    rows = [O.devrng_reset_tuple(cfg["seed"], gid0 + i, 0, ct.S, ct.Y, ct.n_samples, ct.fips_to_weather, ct.sim_ptr,
                                 ct.sim_cnt, True, lambda cw, yi: int(ct.B0[cw * ct.Y + yi]), -1, bkw, mode)
            for i in range(n)]
    cw, cc, yi, sm, b = (np.array(col, np.int64) for col in zip(*rows))
    return dict(county_w=cw, coef_col=cc, year_i=yi, sample=sm, budget=b)


def _sampling_policy(ct):
    """a sampled linear policy that alerts often and runs into the budget (the other gradient tests' prefix policy)"""
    rng = np.random.default_rng(9)
    W = (rng.standard_normal((1, ct.n_obs)) * 0.2).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] *= 0.1
    return W.astype(np.float64)[0], 0.3


def _oracle_at_start(tb, name, c, n, gid0):
    V = tb.oracle()
    E.oracle_reset(V, tuples(tb.ct, RESET[name], n, gid0))
    for day in range(c["prefix"]):
        E.oracle_step(V, prefix_actions(n, day, gid0).astype(np.int64))
    return V


def schedule(tb, name, c, n, gid0=E.GID0):
    """the case's schedule, bool [n, T] by day of the episode. "sampled": the ATTEMPTS of the sampled linear policy
    rolled out by the oracle from where the batch stands after the prefix (attempts go on at the budget)"""
    ct = tb.ct
    if c["sched"] != "sampled":
        return host_schedule(c["sched"], n, ct.T, gid0)
    V = _oracle_at_start(tb, name, c, n, gid0)
    w, b = _sampling_policy(ct)
    uni = lambda t: O.devrng_policy_uniform_vec(19, gid0 + np.arange(n), np.zeros(n, np.int64), t)  # noqa: E731
    R = E.oracle_record(V, lambda obs: (obs.astype(np.float64) @ w + b, np.ones(len(obs))), ct.T, (0.0, 0.0), uniform=uni,
                        T=ct.T)
    assert (V.used >= V.budget).any()  # envs at the budget
    return R["att"]


def oracle_rows(tb, name, c, n, sched, gid0=E.GID0):
    """the case replayed by the NumPy oracle: what the GPU file's stepped twin records (tests/q_restatement.py: q_fp64)"""
    ct = tb.ct
    V = _oracle_at_start(tb, name, c, n, gid0)
    S = ct.T if c["n_steps"] is None else c["n_steps"]
    R = dict(obs=np.zeros((S + 1, n, ct.n_obs)), reward=np.zeros((S, n)), valid=np.zeros((S, n), bool),
             issued=np.zeros((S, n), bool), attempted=np.zeros((S, n), bool), terminal=np.zeros((S, n), bool),
             left_after=np.zeros((S, n), np.int64))
    rows = np.arange(n)
    for s in range(S):
        live = ~V._finished
        R["obs"][s] = V.obs.astype(np.float32)
        act = sched[rows, np.minimum(V.t, ct.T - 1)] & live
        r, done, actual, _ = E.oracle_step(V, act.astype(np.int64))
        R["valid"][s], R["attempted"][s], R["issued"][s] = live, act, live & (actual == 1)
        R["reward"][s], R["terminal"][s] = np.where(live, r, 0.0), live & done
        R["left_after"][s] = V.budget - V.used
    R["obs"][S] = V.obs.astype(np.float32)
    return R
