"""The cases of tests/test_actor_critic_gpu.py, shared with tests/test_actor_critic_cpu.py: which net, table, prefix,
schedule, gate, mode and settings every comparison of actor_critic_gradient() runs, and everything about a case that is
decided on the host -- the two-row nets, the groups, the days before the call, the schedule, the gate, an epoch's three
input arrays. The CPU file replays every case with the NumPy oracle and holds the restatement's own ambiguity shares
under the cap; the GPU file runs the kernels against a twin stepped through step(). Shapes, nets, groups, weights,
prefixes and schedules are those of tests/q_gradient_cases.py; the n_obs = 8 layouts come from tests/obs_layouts.py.
Nothing here touches the GPU or the library."""
import numpy as np

import obs_layouts as L
import q_gradient_cases as QC
from actor_critic_restatement import ac_fp64

N, G = QC.N, QC.G  # 300 envs: four full waves and a partial one; groups 0, 1 and 3 of 4, group 2 empty
GID0 = QC.E.GID0
RESET = dict(QC.RESET, n8=L.RESET["n8"], n8_ragged=L.RESET["n8_ragged"])
INSTANTIATION = QC.INSTANTIATION
# the six <WIDTH, LAYERS> instantiations, every net with padded units ((24, 40) is the padded <64, 2> net)
NETS = ("h7", "h24", "h40", "h7x13", "h24x20", "h24x40")

DEFAULT = dict(table="synth", n=N, prefix=9, n_steps=None, mode="collect", bootstrap=False, gamma=0.99, lam=0.95,
               clip=0.2, vf_coef=0.5, beta=0.01, rb=False, gate=False, sched="random", weights=True, grouped=True,
               order=False)


def make_tables():
    """name -> table: those of tests/q_gradient_cases.py (the 153-day mini table "synth", the 12-day "short", "ragged")
    and the n_obs = 8 layout of tests/obs_layouts.py, rectangular and ragged"""
    out = QC.make_tables()
    out.update(L.make_layouts(("n8", "n8_ragged")))
    return out


def _matrix():
    """every instantiation under both activations and in both modes: net i runs (tanh, collect) and (relu, epoch) for
    even i, the modes swapped for odd i"""
    out = {}
    for i, net in enumerate(NETS):
        for j, act in enumerate(("tanh", "relu")):
            mode = ("collect", "epoch")[(i + j) % 2]
            out[f"{net}_{act}_{mode}"] = dict(net=net, act=act, mode=mode, order=(i + j) % 3 == 1)
    return out


CASES = _matrix()
CASES.update({
    # require_budget on a schedule that runs into the budget: forced days with no policy score
    "h24x20_tanh_epoch_at_budget": dict(net="h24x20", act="tanh", mode="epoch", rb=True, sched="sampled"),
    "h7x13_relu_collect_at_budget": dict(net="h7x13", act="relu", rb=True, sched="sampled", gamma=1.0, lam=1.0),
    # the gate: closed days are forced choices, the value term stays
    "h24_tanh_collect_gated": dict(net="h24", act="tanh", gate=True, rb=True),
    "h24x40_relu_epoch_gated": dict(net="h24x40", act="relu", mode="epoch", gate=True, order=True),
    # chunks: n_steps < T with and without the bootstrap
    "h40_tanh_collect_n3_bootstrap": dict(net="h40", act="tanh", n_steps=3, bootstrap=True, gamma=0.9, lam=0.8),
    "h64x64_relu_collect_n1": dict(net="h64x64", act="relu", n_steps=1),
    "h64x64_tanh_epoch_n3": dict(net="h64x64", act="tanh", mode="epoch", n_steps=3),
    # the ragged table (envs finished on entry) and the n_obs = 8 layouts
    "h40_relu_collect_ragged": dict(net="h40", act="relu", table="ragged", prefix=25),
    "h7_tanh_epoch_ragged": dict(net="h7", act="tanh", table="ragged", prefix=25, mode="epoch"),
    "h24x20_relu_collect_n8": dict(net="h24x20", act="relu", table="n8", prefix=5),
    "h7x13_tanh_epoch_n8": dict(net="h7x13", act="tanh", table="n8", prefix=5, mode="epoch", gate=True),
    "h24_relu_collect_n8_ragged_bootstrap": dict(net="h24", act="relu", table="n8_ragged", prefix=0, n_steps=7,
                                                 bootstrap=True),
    "h24_tanh_epoch_one_group_no_weights": dict(net="h24", act="tanh", mode="epoch", grouped=False, weights=False, prefix=0),
})
# the six instantiations at 3 tiles per wave: 131 272 envs on the 12-day table, groups of 1 000 consecutive env ids, the
# groups of QC.CHECKED rebuilt as small batches with the same global env ids
LARGE = {f"{net}_{act}_{mode}_large": dict(net=net, act=act, mode=mode)
         for i, net in enumerate(NETS) for act, mode in ((("relu", "collect"), ("tanh", "epoch"))[i % 2],)}
LARGE_DEFAULT = dict(DEFAULT, table="short", n=QC.N_LARGE, prefix=2, sched="dense")


def case(name):
    return dict(DEFAULT, **CASES[name]) if name in CASES else dict(LARGE_DEFAULT, **LARGE[name])


def steps(ct, c):
    return ct.T if c["n_steps"] is None else c["n_steps"]


def net(ct, c, G_):
    """[(W [G_, out, in], b [G_, out]), ...]: row 0 the policy logit, row 1 the state value"""
    return QC.qnet(ct, c["net"], G_)


def policy_dict(layers, c, g=None, allowed=None):
    p = dict(kind="mlp", layers=layers, activation=c["act"], require_budget=c["rb"])
    if g is not None:
        p["group"] = g
    if allowed is not None:
        p["allowed_days"] = allowed
    return p


def gate(n, T, gid0=GID0):
    """bool [n, T] by day of the episode, a function of the global env id: 70 % of the days open"""
    gid = gid0 + np.arange(n, dtype=np.uint64)[:, None]
    h = (gid * np.uint64(40503) + np.arange(T, dtype=np.uint64)[None, :] * np.uint64(2654435761)) % np.uint64(1000)
    return h < np.uint64(700)


def epoch_inputs(S, n, lo=0, nk=None):
    """(advantage, value_target, old_log_prob) f32 [S, n] by call-day and env id: advantages of both signs with zeros,
    targets around the rewards' scale, log-probabilities between -2 and -0.05 -- against the net's own lp_s that is a
    ratio on either side of both clip edges, so some days clip and some do not. Drawn for the whole batch and sliced
    (lo, nk), so that a small batch rebuilt from a large one reads the same numbers."""
    rng = np.random.default_rng(31)
    A = rng.standard_normal((S, n)).astype(np.float32)
    A[:, ::11] = 0.0
    T = (0.5 * rng.standard_normal((S, n)) - 0.5).astype(np.float32)
    old = (-0.05 - 1.95 * rng.random((S, n)) ** 2).astype(np.float32)
    sl = slice(lo, lo + (n - lo if nk is None else nk))
    return A[:, sl], T[:, sl], old[:, sl]


def schedule(tb, c, n, gid0=GID0):
    return QC.schedule(tb, c["table"], dict(c, prefix=c["prefix"]), n, gid0)


def oracle_rows(tb, c, n, sched, allowed=None, gid0=GID0):
    """The case replayed by the NumPy oracle: what the GPU file's stepped twin records (actor_critic_restatement.ac_fp64).
    A forced day (require_budget with nothing left, or a closed day) is attempted as 0."""
    ct = tb.ct
    V = tb.oracle()
    QC.E.oracle_reset(V, QC.tuples(ct, RESET[c["table"]], n, gid0))
    for day in range(c["prefix"]):
        QC.E.oracle_step(V, QC.prefix_actions(n, day, gid0).astype(np.int64))
    S = steps(ct, c)
    R = dict(obs=np.zeros((S + 1, n, ct.n_obs)), reward=np.zeros((S, n)),
             **{k: np.zeros((S, n), bool) for k in ("valid", "labels", "forced", "issued", "terminal")})
    rows = np.arange(n)
    for s in range(S):
        live = ~V._finished
        tt = np.minimum(V.t, ct.T - 1)
        R["obs"][s] = V.obs.astype(np.float32)
        R["valid"][s], R["labels"][s] = live, sched[rows, tt] & live
        forced = np.zeros(n, bool) if allowed is None else ~allowed[rows, tt]
        if c["rb"]:
            forced |= (V.budget - V.used) <= 0
        R["forced"][s] = forced & live
        r, done, actual, _ = QC.E.oracle_step(V, (R["labels"][s] & ~R["forced"][s]).astype(np.int64))
        R["issued"][s], R["terminal"][s] = live & (actual == 1), live & done
        R["reward"][s] = np.where(live, r, 0.0)
    R["obs"][S] = V.obs.astype(np.float32)
    return R


def restate(c, R, w, layers, g, n_groups, inputs=None, **extra):
    """ac_fp64 on a walk's rows (the oracle's, or the stepped twin's); inputs: an epoch's three arrays"""
    kw = dict(clip=c["clip"], vf_coef=c["vf_coef"], beta=c["beta"])
    if inputs is None:
        kw.update(gamma=c["gamma"], lam=c["lam"], bootstrap=c["bootstrap"])
    else:
        kw.update(advantage=inputs[0], value_target=inputs[1], old_log_prob=inputs[2])
    kw.update(extra)
    return ac_fp64(R["obs"], R["labels"], R["valid"], R["forced"], R["terminal"], R["reward"], w, layers, c["act"], g,
                   n_groups, **kw)


def not_trivial(c, R, ref, what):
    """a case that scores nothing, clips nothing or everything, or never forces a day where it should proves little"""
    m, valid = ref["m"], R["valid"]
    assert m.any() and (m & R["labels"]).any() and (m & ~R["labels"]).any(), what  # alerts and non-alerts are scored
    assert (np.abs(ref["c_pi"])[m] > 0).any() and (np.abs(ref["c_v"])[valid] > 0).any(), what
    if c["mode"] == "epoch":
        assert (m & ~ref["live"]).any() and (m & ref["live"] & (ref["rho"] != 1.0)).any(), what  # some days clip, some do not
    if c["rb"] or c["gate"]:
        assert (valid & R["forced"]).any() and (np.abs(ref["c_v"])[valid & R["forced"]] > 0).any(), what
        assert (ref["c_pi"][valid & R["forced"]] == 0).all(), what
