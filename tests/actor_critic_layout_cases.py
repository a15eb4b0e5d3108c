"""The cases of tests/test_actor_critic_layouts_gpu.py, shared with tests/test_actor_critic_layouts_cpu.py: which table,
net, activation, mode, prefix, schedule, gate and settings every comparison of actor_critic_gradient() runs on the
observation layouts of tests/obs_layouts.py (columns off their index, empty slots, n_obs of 29, 28, 8 and 5, run-time
slots in reverse order, two ragged variants) and on the slot-27 tables of tests/table_edges.py. Nothing is restated here:
the tables, episode tuples, reset settings and the oracle's walk (with the fp64 all-slot rewards on the slot-27 tables)
are those of tests/obs_layout_learner_cases.py; the nets, groups, weights, prefix actions and schedules those of
tests/q_gradient_cases.py; the gate, an epoch's inputs, the policy dict, the restatement call and the non-triviality
conditions those of tests/actor_critic_cases.py. Nothing here touches the GPU or the library's kernels."""
import numpy as np

import actor_critic_cases as AC
import obs_layout_learner_cases as C
import obs_layouts as L
import q_gradient_cases as QC
import table_edges as E

N, N27 = C.N, C.N27  # 193 envs on the layouts (three full waves and a partial one), 300 on the slot-27 tables
G = QC.G  # groups 0, 1 and 3 of 4, group 2 empty
GID0 = E.GID0
ORDER = C.ORDER
NETS = AC.NETS  # the six <WIDTH, LAYERS> instantiations, every net with padded units
TABLES = C.ALL + C.SLOT27
RAGGED = L.RAGGED + ("ragged27",)
BITS_TABLES = ("permuted", "narrow", "slot27")  # bit equality with the one-head kernels
ONE_COLUMN = C.ONE_COLUMN  # permuted, n8, narrow
# case id -> shift of the schedule's hash: moved when a case's ambiguity share (clip-edge bands, ReLU kinks) leaves the
# restatement's cap (tests/test_actor_critic_layouts_cpu.py); the cap stays, the seed moves. None needs it.
SEEDS = {}

DEFAULT = dict(AC.DEFAULT, table=None, n=N, prefix=5, n_steps=None)


def _case(net, act, mode, table, tag="", **kw):
    c = dict(DEFAULT, net=net, act=act, mode=mode, table=table, n=N27 if table in C.SLOT27 else N)
    c.update(kw)
    c["id"] = f"{net}_{act}_{mode}_{table}" + (f"_{tag}" if tag else "")
    return c


def _matrix():
    """every table in both modes; case k = 2 * table + mode runs net k mod 6, the activation alternating with the net and
    swapped on the second round, so the first twelve cases are the twelve (instantiation, activation) pairs; each table
    runs one mode on the identity visiting order and the other on the handle's own. The ragged tables collect from
    reset (the 1-, 2- and 3-day episodes are walked from their first day) and run their epoch after the prefix (envs
    finished on entry)."""
    out = []
    for ti, table in enumerate(TABLES):
        for mi, mode in enumerate(("collect", "epoch")):
            k = 2 * ti + mi
            kw = dict(order=(ti + mi) % 2 == 1)
            if table in RAGGED and mode == "collect":
                kw["prefix"] = 0
            out.append(_case(NETS[k % 6], ("tanh", "relu")[(k // 6 + k % 6) % 2], mode, table, **kw))
    return out


def all_cases():
    out = _matrix()
    # the gate: closed days are forced choices, the value term stays
    # (ragged27 draws its budgets in [0, default]: require_budget there would leave few scored days, so it joins the
    # gate on permuted)
    out.append(_case("h24x40", "relu", "epoch", "permuted", "gated", gate=True, rb=True, order=True))
    out.append(_case("h24", "tanh", "collect", "ragged27", "gated", gate=True, gamma=1.0, lam=1.0))
    # require_budget on a schedule that runs into the budget: forced days with no policy score
    out.append(_case("h24x20", "tanh", "epoch", "n28", "at_budget", rb=True, sched="sampled"))
    out.append(_case("h7x13", "relu", "collect", "slot27", "at_budget", rb=True, sched="sampled", gamma=1.0, lam=1.0,
                     order=True))
    # a 7-day chunk from reset with the bootstrap on every ragged table: episodes end inside it, others run on
    out.append(_case("h40", "tanh", "collect", "permuted_ragged", "n7_bootstrap", prefix=0, n_steps=7, bootstrap=True,
                     gamma=0.9, lam=0.8, order=True))
    out.append(_case("h24", "relu", "collect", "n8_ragged", "n7_bootstrap", prefix=0, n_steps=7, bootstrap=True))
    out.append(_case("h7x13", "tanh", "collect", "ragged27", "n7_bootstrap", prefix=0, n_steps=7, bootstrap=True,
                     gamma=0.9, lam=0.8))
    return out


CASES = {c["id"]: c for c in all_cases()}
make_tables, reset_cfg, tuples = C.make_tables, C.reset_cfg, C.tuples
steps, net, policy_dict, restate, not_trivial, epoch_inputs = (AC.steps, AC.net, AC.policy_dict, AC.restate, AC.not_trivial,
                                                               AC.epoch_inputs)


def groups(c):
    return QC.groups(c["n"])


def weights(c):
    return QC.weights(c["n"]) if c["weights"] else None


def gate(tb, c):
    """bool [n, T] or None: actor_critic_cases.gate, 70 % of the days open"""
    return AC.gate(c["n"], tb.ct.T, GID0) if c["gate"] else None


def schedule(tb, c):
    """obs_layout_learner_cases.schedule with this file's seeds: bool [n, T] by day of the episode. "random": 35 % of the
    days (q_gradient_cases.host_schedule); "sampled": the attempts of q_gradient_cases' sampled linear policy rolled out
    by the oracle from where the batch stands after the prefix, which go on at the budget"""
    ct, n = tb.ct, c["n"]
    gid0 = GID0 + SEEDS.get(c["id"], 0)
    if c["sched"] != "sampled":
        return QC.host_schedule(c["sched"], n, ct.T, gid0)
    V = C.oracle_at_start(tb, c)
    w, b = QC._sampling_policy(ct)
    uni = lambda t: QC.O.devrng_policy_uniform_vec(19, gid0 + np.arange(n), np.zeros(n, np.int64), t)  # noqa: E731
    R = E.oracle_record(V, lambda obs: (obs.astype(np.float64) @ w + b, np.ones(len(obs))), ct.T, (0.0, 0.0), uniform=uni,
                        T=ct.T)
    assert (V.used >= V.budget).any()  # envs at the budget
    return R["att"]


def inputs(tb, c):
    """an epoch's (advantage, value_target, old_log_prob), or None for a collect case"""
    return AC.epoch_inputs(steps(tb.ct, c), c["n"]) if c["mode"] == "epoch" else None


def walk(tb, c, sched=None):
    """the case on the NumPy oracle: obs_layout_learner_cases.oracle_walk (the fp64 all-slot rewards on slot-27 tables)"""
    sched = schedule(tb, c) if sched is None else sched
    return C.oracle_walk(tb, c, sched, force_rb=c["rb"], allowed=gate(tb, c))


def reference(tb, c, R, layers=None, w="case"):
    """the fp64 restatement on a walk's rows (the oracle's, or the stepped twin's)"""
    layers = net(tb.ct, c, G) if layers is None else layers
    return restate(c, R, weights(c) if isinstance(w, str) else w, layers, groups(c), G, inputs(tb, c))


def ambiguity(ref):
    return ref["ambiguous_share"] + ref["near_kink"] + ref["near_tie"]


# ------------------------------------------------------------------ one column alone
# the case each table's one-column net runs under: both modes, both activations, <16, 1> and <64, 2>
ONE_COLUMN_CASES = {"permuted": "h7_tanh_collect_permuted", "n8": "h24x40_relu_epoch_n8", "narrow": "h7_relu_collect_narrow"}
ONE_COLUMN_SHIFT = 0.5


def one_column(ct):
    """obs_layout_learner_cases.one_column: a table column off its index, `remaining_budget` (slot 26) on narrow"""
    return C.one_column(ct)


def zero_columns(R):
    """the observation columns that are 0 on every stepped day of a walk"""
    S = R["valid"].shape[0]
    x = R["obs"][:S][R["valid"]]
    return [j for j in range(x.shape[1]) if not x[:, j].any()]


def one_column_net(ct, c, col, shift=0.0):
    """the case's net with a first layer that is zero except on observation column `col`: there the drawn weights' signs
    at 1 + |w| times obs_layout_learner_cases.column_scale (so the column moves the hidden units over its own range),
    plus `shift` column scales on every unit"""
    layers = [(W.copy(), b.copy()) for W, b in net(ct, c, G)]
    scale = C.column_scale(ct, col)
    W0 = layers[0][0]
    W1 = np.zeros_like(W0)
    W1[:, :, col] = scale * (np.sign(W0[:, :, col]) * (1.0 + np.abs(W0[:, :, col])) + np.float32(shift))
    layers[0] = (W1, layers[0][1])
    return layers
