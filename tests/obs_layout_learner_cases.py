"""The cases of tests/test_obs_layouts_learners_gpu.py, shared with tests/test_obs_layouts_learners_cpu.py: which table,
net, groups, prefix, schedule and settings every comparison of value_gradient() (plain and GAE), surrogate_gradient(),
fisher_vector_product(), q_gradient() and alert_gate() runs on the observation layouts of tests/obs_layouts.py and on the
slot-27 tables of tests/table_edges.py, and everything about a case that is decided on the host: parameters, groups,
the days before the call, the schedule, the weights, the walk of the NumPy oracle along the schedule and the call of the
entry point's fp64 restatement on a walk's rows. The GPU file walks a twin through step() instead and hands its rows to
the same restatement. Nothing here touches the GPU or the library's kernels."""
import numpy as np

import obs_layouts as L
import q_gradient_cases as QC
import table_edges as E
from alert_gate_restatement import gate_fp32
from fisher_restatement import fisher_linear_fp64, fisher_mlp_fp64
from gae_restatement import gae_linear_fp64, gae_mlp_fp64
from policy_gradient_mlp_cases import MATRIX, net as case_net
from posterior_restatement import posterior_returns_fp64
from q_restatement import q_fp64
from surrogate_restatement import surrogate_linear_fp64, surrogate_mlp_fp64
from value_gradient_restatement import value_linear_fp64, value_mlp_fp64

N = 193  # three full waves and a partial one
N27 = 300  # the slot-27 tables
ALL = L.LAYOUTS + L.RAGGED
SLOT27 = ("slot27", "ragged27")
# nets of the instantiation matrix that between them reach widths 16, 32 and 64 and both layer counts
PG_NETS = ("tanh7x13", "relu29_o2", "relu40x64")
IM_NETS = ("tanh1_o2", "tanh64x33_o2")  # <16, 1> and <64, 2>
Q_NETS = ("h7", "h24x20", "h64x64")  # <16, 1>, <32, 2>, <64, 2>
ORDER = dict(lockstep=False, rollout_order=True)  # the handle's visiting order: not the identity
GAE = (0.97, 0.9)
CLIP, BETA = 0.2, 0.01
# case id -> shift of the schedule's hash: moved when a case's ambiguity share (near ties, ReLU kinks) leaves the
# restatement's cap (tests/test_obs_layouts_learners_cpu.py); the cap stays, the seed moves. None needs it.
SEEDS = {}


def make_tables():
    """name -> table_edges.Table: the six layouts and the two slot-27 tables"""
    out = L.make_layouts()
    out.update({k: v for k, v in E.make_tables().items() if k in SLOT27})
    return out


def reset_cfg(name):
    return L.RESET[name] if name in L.RESET else E.RESET[name]


_TUPLES = {}


def tuples(tb, n):
    """the episode tuples the table's reset draws for n envs (computed once per table and env count, left unchanged)"""
    key = (tb.name, n)
    if key not in _TUPLES:
        _TUPLES[key] = E.host_tuples(tb, n, reset_cfg(tb.name))
    return _TUPLES[key]


# ------------------------------------------------------------------ the cases
def _case(entry, table, kind, i, **kw):
    c = dict(entry=entry, table=table, kind=kind, n=N, prefix=0, order=i % 2 == 1, rb=False, n_steps=None, bootstrap=False,
             gate=False, sched="random", weights=True)
    c.update(kw)
    c["id"] = f"{entry}-{table}-{kind}" + ("-gated" if c["gate"] else "")
    return c


def _layers_of(kind):
    return len(MATRIX[kind][1]) if kind in MATRIX else 0


def value_cases(entry):
    """"value": the plain path (gamma = lambda = 1, no bootstrap; k_vg_*); "gae": (0.97, 0.9), a 7-day chunk with the
    bootstrap on the ragged layouts (k_gae_*). From reset for the one-layer nets, after a 9-day prefix for the others."""
    out = []
    for li, name in enumerate(ALL):
        for ki, kind in enumerate(("linear",) + PG_NETS):
            kw = dict(prefix=0 if _layers_of(kind) == 1 else 9)
            if entry == "gae" and name in L.RAGGED:
                kw.update(n_steps=7, bootstrap=True)
            out.append(_case(entry, name, kind, li + ki, **kw))
    return out


def surrogate_cases():
    return [_case("surrogate", name, kind, li + ki, prefix=5, rb=((li + 1) // 2 + ki) % 2 == 1)
            for li, name in enumerate(ALL) for ki, kind in enumerate(("linear",) + IM_NETS)]


def fisher_cases():
    out = [_case("fisher", name, kind, li + ki, prefix=9, rb=((li + 1) // 2 + ki) % 2 == 1)
           for li, name in enumerate(ALL) for ki, kind in enumerate(("linear",) + PG_NETS)]
    return out + [_case("fisher", "ragged27", "linear", 1, n=N27, prefix=9, rb=True)]


def q_cases():
    """the six layouts under <16, 1>, <32, 2> and <64, 2>, and the two slot-27 tables under h40 (ReLU, double) and h7x13
    (tanh), whole episodes"""
    out = []
    for li, name in enumerate(ALL):
        for ni, net in enumerate(Q_NETS):
            k = li * 3 + ni
            sampled = net == "h24x20"
            kw = dict(act=("tanh", "relu")[(li + ni) % 2], target=(li + ni) % 3 != 2, double=(k // 2) % 2 == 1, rb=sampled,
                      sched="sampled" if sampled else "random", loss=("huber", "huber", "squared")[k % 3],
                      huber_delta=(2.0, 4.0)[(k // 3) % 2], gamma=0.99, prefix=(0, 12, 9)[ni])
            if name in L.RAGGED:
                kw.update(n_steps=5, bootstrap=True)
            out.append(_case("q", name, net, (li + 1) // 2 + ni, **kw))
    for ti, name in enumerate(SLOT27):
        out.append(_case("q", name, "h40", ti, n=N27, act="relu", target=True, double=True, loss="huber", huber_delta=4.0,
                         gamma=0.99))
        out.append(_case("q", name, "h7x13", ti + 1, n=N27, act="tanh", target=ti == 0, double=False, loss="squared",
                         huber_delta=2.0, gamma=0.9))
    return out


def gated_cases():
    """"allowed_days" from alert_gate("heat_qi", the column's median) on permuted and n8_ragged"""
    out = []
    for li, name in enumerate(("permuted", "n8_ragged")):
        for entry, net in (("surrogate", IM_NETS[1]), ("fisher", PG_NETS[0])):
            for ki, kind in enumerate(("linear", net)):
                out.append(_case(entry, name, kind, li + ki, prefix=5, rb=ki == 1, gate=True))
    return out


def all_cases():
    return value_cases("value") + value_cases("gae") + surrogate_cases() + fisher_cases() + q_cases() + gated_cases()


def by_id(cases):
    return {c["id"]: c for c in cases}


# ------------------------------------------------------------------ what a case decides on the host
def n_groups(c):
    return QC.G if c["entry"] == "q" else E.G


def groups(c):
    """q_gradient: groups 0, 1 and 3 of 4 (group 2 empty: NaN rows); the others: table_edges' five interleaved groups"""
    return QC.groups(c["n"]) if c["entry"] == "q" else E.groups(c["n"])


def weights(c):
    return QC.weights(c["n"]) if c["weights"] else None  # zeros and negative values


def steps(ct, c):
    return ct.T if c["n_steps"] is None else c["n_steps"]


def params(ct, c):
    """the policy / value / Q-net dict of the case (numpy parameters, the group array, require_budget), and for
    q_gradient the target net's dict or None"""
    g = groups(c)
    if c["entry"] == "q":
        q = dict(kind="mlp", layers=QC.qnet(ct, c["kind"], QC.G), activation=c["act"], group=g, require_budget=c["rb"])
        tg = dict(kind="mlp", layers=QC.qnet(ct, c["kind"], QC.G, seed_shift=1), activation=c["act"], group=g) if c["target"] else None
        return q, tg
    if c["kind"] == "linear":
        W, b = E.linear_params(ct)
        pol = dict(kind="linear", weight=W, bias=b, group=g)
    else:
        _, hidden, act, n_out = MATRIX[c["kind"]]
        pol = dict(kind="mlp", layers=case_net(ct, c["kind"], hidden, n_out), activation=act, group=g)
    if c["entry"] in ("surrogate", "fisher"):
        pol["require_budget"] = c["rb"]
    return pol, None


def _perturb(arrays, seed, size=0.3):
    rng = np.random.default_rng(seed)
    return [(x + size * np.abs(x).mean() * rng.standard_normal(x.shape)).astype(np.float32) for x in arrays]


def perturbed(pol, seed=77):
    """the "old" policy of the surrogate's ratios (as tests/test_surrogate_gpu.py): some days clip, some do not"""
    if pol["kind"] == "linear":
        W, b = _perturb([pol["weight"], pol["bias"]], seed)
        return dict(pol, weight=W, bias=b)
    Ws, bs = _perturb([W for W, _ in pol["layers"]], seed), _perturb([b for _, b in pol["layers"]], seed + 1)
    return dict(pol, layers=list(zip(Ws, bs)))


def advantage(S, n, seed=31):
    """both signs, zeros, magnitudes around 1 (as tests/test_surrogate_gpu.py)"""
    A = np.random.default_rng(seed).standard_normal((S, n)).astype(np.float32)
    A[:, ::11] = 0.0
    return A


def vector(pol, seed=41):
    """a random vector in the shape of the policy's gradient (as tests/test_fisher_gpu.py)"""
    rng = np.random.default_rng(seed)
    if pol["kind"] == "linear":
        return {"weight": rng.standard_normal(pol["weight"].shape).astype(np.float32),
                "bias": rng.standard_normal(pol["bias"].shape).astype(np.float32)}
    return {"layers": [(rng.standard_normal(np.shape(W)).astype(np.float32) / np.float32(np.sqrt(np.shape(W)[-1])),
                        rng.standard_normal(np.shape(b)).astype(np.float32)) for W, b in pol["layers"]]}


def prefix_actions(c):
    """the attempts of the days before the call, int32 [prefix, n]"""
    return [QC.prefix_actions(c["n"], day) for day in range(c["prefix"])]


def oracle_at_start(tb, c):
    V = tb.oracle()
    E.oracle_reset(V, tuples(tb, c["n"]))
    for a in prefix_actions(c):
        E.oracle_step(V, a.astype(np.int64))
    return V


def schedule(tb, c):
    """bool [n, T] by day of the episode. "random": 35 % of the days, a function of the env id; "sampled": the ATTEMPTS of
    the sampled linear policy of tests/q_gradient_cases.py rolled out by the oracle from where the batch stands after the
    prefix (attempts go on at the budget)"""
    ct, n = tb.ct, c["n"]
    gid0 = E.GID0 + SEEDS.get(c["id"], 0)
    if c["sched"] != "sampled":
        return QC.host_schedule(c["sched"], n, ct.T, gid0)
    V = oracle_at_start(tb, c)
    w, b = QC._sampling_policy(ct)
    uni = lambda t: QC.O.devrng_policy_uniform_vec(19, gid0 + np.arange(n), np.zeros(n, np.int64), t)  # noqa: E731
    R = E.oracle_record(V, lambda obs: (obs.astype(np.float64) @ w + b, np.ones(len(obs))), ct.T, (0.0, 0.0), uniform=uni,
                        T=ct.T)
    assert (V.used >= V.budget).any()  # envs at the budget
    return R["att"]


# ------------------------------------------------------------------ the alert gate
def gate_start(tup, t, finished):
    """what gate_fp32 reads of a state: t and finished of the moment, the rest from the episode tuples"""
    return dict(t=np.asarray(t, np.int64), finished=np.asarray(finished).astype(np.int64), n_days=tup["n_days"],
                county_w=tup["county_w"], year_i=tup["year_i"])


def gate_columns(ct):
    """the observation columns alert_gate() is checked on: heat_qi and obs_layouts.offset_column where there is one"""
    cols = [ct.feature_names.index("heat_qi")]
    c = L.offset_column(ct)
    return cols + ([] if c is None else [c])


def _median(x):
    """the median, or for a column whose median is its smallest value (a 0 / 1 flag that is mostly 0: `>=` the median
    would leave every day open) the midpoint of its range"""
    m = float(np.median(x))
    return m if m > float(x.min()) else 0.5 * (float(x.min()) + float(x.max()))


def gate_thresholds(ct, tup, col):
    """(scalar, float32 [n]): the median of the column over the batch's own episode days, and every env's own median"""
    slot = ct.obs_slot[col]
    row = tup["county_w"] * ct.Y + tup["year_i"]
    X = np.asarray(ct.X)
    per_env = np.array([_median(X[:tup["n_days"][e], row[e], slot]) for e in range(len(row))], np.float32)
    live = np.arange(ct.T)[:, None] < tup["n_days"][None, :]
    return float(np.float32(_median(X[:, row, slot][live]))), per_env


def gate_mask(tb, c, V):
    """the case's "allowed_days" from the restatement: alert_gate("heat_qi", the column's median) where `V` stands"""
    ct, tup = tb.ct, tuples(tb, c["n"])
    col = ct.feature_names.index("heat_qi")
    tau, _ = gate_thresholds(ct, tup, col)
    return gate_fp32(ct.X, ct.Y, ct.obs_slot[col], gate_start(tup, V.t, V._finished), tau), tau


# ------------------------------------------------------------------ the walk along the schedule
def new_rows(S, n, n_obs):
    R = dict(obs=np.zeros((S + 1, n, n_obs)), reward=np.zeros((S, n)), left_after=np.zeros((S, n), np.int64),
             count14=np.zeros((S, n), np.int64))
    R.update({k: np.zeros((S, n), bool) for k in ("valid", "labels", "forced", "closed", "issued", "terminal")})
    return R


def oracle_walk(tb, c, sched, force_rb=False, allowed=None, V=None):
    """The case replayed by the NumPy oracle from where it stands after the prefix: what the GPU file's stepped twin
    records. obs f64 [S + 1, n, n_obs] (slab s: the f32 row held before decision s; slab S: the row the call leaves
    behind), reward f64, left_after (budget - used after day s), count14 (the 14-day alert count in the row of day s),
    valid / labels (the schedule's attempts) / forced (require_budget with nothing left, or a closed day) / closed /
    issued / terminal bool [S, n], alive bool [n]. A forced day's attempt is 0. On the slot-27 tables the oracle's
    rewards lack the slot-27 term: they are replaced by the fp64 restatement of the reward with every slot."""
    ct, n = tb.ct, c["n"]
    V = oracle_at_start(tb, c) if V is None else V
    S = steps(ct, c)
    R = new_rows(S, n, ct.n_obs)
    rows, a2w = np.arange(n), ct.feature_names.index("alert_2wks")
    start = dict(E.start_state(tuples(tb, n)), t=V.t.copy(), used=V.used.copy(), streak=V.streak.copy(),
                 hist14=E.oracle_state(V)["hist14"], finished=V._finished.astype(np.int64), sample=tuples(tb, n)["sample"])
    days = np.zeros((n, ct.T), bool)
    for s in range(S):
        live = ~V._finished
        R["obs"][s] = V.obs.astype(np.float32)
        tt = np.minimum(V.t, ct.T - 1)
        R["valid"][s], R["labels"][s] = live, sched[rows, tt] & live
        if allowed is not None:
            R["closed"][s] = ~allowed[rows, tt] & live
        R["forced"][s] = (R["closed"][s] | (force_rb & ((V.budget - V.used) <= 0))) & live
        R["count14"][s] = V.obs[:, a2w]
        r, done, actual, _ = E.oracle_step(V, (R["labels"][s] & ~R["forced"][s]).astype(np.int64))
        R["issued"][s], R["terminal"][s] = live & (actual == 1), live & done
        R["reward"][s] = np.where(live, r, 0.0)
        R["left_after"][s] = V.budget - V.used
        days[rows[R["issued"][s]], tt[R["issued"][s]]] = True
    R["obs"][S] = V.obs.astype(np.float32)
    R["alive"] = ~V._finished
    if tb.slot27:
        _, per_day = posterior_returns_fp64(ct.X, ct.W, ct.n_samples, ct.Y, start, days, S, per_day=True)
        r = per_day[rows, :, start["sample"]].T
        assert (np.isnan(r) == ~R["valid"]).all()
        known = ~tb.a2w[start["coef_col"]]  # where the oracle has every coefficient the two agree
        assert np.abs(np.where(R["valid"], r - R["reward"], 0.0))[:, known].max() <= 1e-9
        R["reward"] = np.where(R["valid"], r, 0.0)
    return R


def reference(c, R, pol, target=None, lp_old=None, vec=None, w="case"):
    """the entry point's fp64 restatement on a walk's rows (the oracle's, or the stepped twin's)"""
    S = R["valid"].shape[0]
    g, G = groups(c), n_groups(c)
    w = weights(c) if isinstance(w, str) else w
    obs = R["obs"]
    lin = pol["kind"] == "linear"
    if c["entry"] == "value":
        if lin:
            return value_linear_fp64(obs[:S], R["valid"], R["reward"], w, pol["weight"], pol["bias"], g, G)
        return value_mlp_fp64(obs[:S], R["valid"], R["reward"], w, pol["layers"], pol["activation"], g, G)
    if c["entry"] == "gae":
        kw = dict(gamma=GAE[0], lam=GAE[1], bootstrap=c["bootstrap"])
        if lin:
            return gae_linear_fp64(obs, R["valid"], R["reward"], R["alive"], w, pol["weight"], pol["bias"], g, G, **kw)
        return gae_mlp_fp64(obs, R["valid"], R["reward"], R["alive"], w, pol["layers"], pol["activation"], g, G, **kw)
    if c["entry"] == "surrogate":
        A = advantage(S + 2, c["n"]).astype(np.float64)
        args = (obs[:S], R["labels"], R["valid"], R["forced"], w, A, lp_old, CLIP, BETA)
        if lin:
            return surrogate_linear_fp64(*args, pol["weight"], pol["bias"], g, G)
        return surrogate_mlp_fp64(*args, pol["layers"], pol["activation"], g, G)
    if c["entry"] == "fisher":
        args = (obs[:S], R["labels"], R["valid"], R["forced"], w)
        if lin:
            return fisher_linear_fp64(*args, pol["weight"], pol["bias"], vec["weight"], vec["bias"], g, G)
        return fisher_mlp_fp64(*args, pol["layers"], vec["layers"], pol["activation"], g, G)
    assert c["entry"] == "q"
    return q_fp64(obs, R["issued"], R["valid"], R["terminal"], R["reward"], R["left_after"], w, pol["layers"],
                  None if target is None else target["layers"], c["act"], g, G, gamma=c["gamma"], double=c["double"],
                  loss=c["loss"], huber_delta=c["huber_delta"], bootstrap=c["bootstrap"], require_budget=c["rb"])


def ambiguity(c, ref):
    """the share every comparison holds under the restatement's cap"""
    if c["entry"] == "q":
        return ref["near_tie"] + ref["near_kink"]
    return ref.get("ambiguous_share", 0.0) + ref.get("near_kink", 0.0)


def forces_on_budget(c):
    """whether the walk marks days without budget as forced (require_budget of the policy kinds; q_gradient's
    require_budget masks the next row's maximum instead, and the critic ignores it)"""
    return c["rb"] and c["entry"] in ("surrogate", "fisher")


# ------------------------------------------------------------------ one column alone
ONE_COLUMN = ("permuted", "n8", "narrow")


def one_column(ct):
    """obs_layouts.offset_column, or `remaining_budget` where the layout has none (narrow)"""
    c = L.offset_column(ct)
    return ct.feature_names.index("remaining_budget") if c is None else c


def column_scale(ct, col):
    slot = ct.obs_slot[col]
    x = np.asarray(ct.X)[:, :, slot].ravel() if slot < 24 else np.array([0.0, 6.0])
    return 2.0 / max(float(x.max() - x.min()), 1e-3)


def one_column_params(ct, entry, col):
    """parameters that are zero except on observation column `col` (and the biases): the linear policy / critic (and the
    Fisher product's vector), or h7's first layer with the other layers as drawn"""
    scale = column_scale(ct, col)
    if entry == "q":
        layers = [(W.copy(), b.copy()) for W, b in QC.qnet(ct, "h7", QC.G)]
        W1 = np.zeros_like(layers[0][0])
        W1[:, :, col] = scale * np.sign(layers[0][0][:, :, col]) * (1.0 + np.abs(layers[0][0][:, :, col]))
        layers[0] = (W1, layers[0][1])
        return layers
    W = np.zeros((E.G, ct.n_obs), np.float32)
    W[:, col] = scale * np.linspace(0.5, 1.5, E.G)
    b = np.linspace(-0.6, 0.2, E.G).astype(np.float32)
    vW = np.zeros_like(W)
    vW[:, col] = np.linspace(1.0, -1.0, E.G) + 0.3
    return W, b, vW, np.linspace(0.4, -0.4, E.G).astype(np.float32)
