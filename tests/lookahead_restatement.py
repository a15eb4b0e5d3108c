"""The lookahead inputs of policy["lookahead"], restated on the host from the compiled tables' own arrays and a state()
dict, and the `a = policy(cat(obs, f)); step(a)` loop on a twin env (tests/test_lookahead_cpu.py,
tests/test_lookahead_gpu.py). Nothing here calls HeatAlertVecEnv.lookahead_features() or lookahead_table().

    f_k = h(r + k) - h(r),  k = 1..D,   r = max(t - 1, 0),   f_k = 0 where r + k >= n_days of the env

h(d): the f32 value of the feature's slot in row (day d, county_w * Y + year_i) of CompiledTables.X; the difference is
one f32 subtraction. The policies are evaluated as tests/test_linear_policy_gpu.py and tests/test_mlp_policy_gpu.py
evaluate theirs (fp64 logits of the f32 parameters), with those files' near-tie rules and their 1 % cap."""
import numpy as np

import table_edges as E
from oracle import heatalert_oracle as O

TIE_CAP = 0.01  # tests/test_linear_policy_gpu.py, tests/test_mlp_policy_gpu.py: near-tie envs stay below 1 %


def tie_bounds(ct, kind):
    """(relative bound on |logit|, bound on |sigmoid - u|) of the reference tests, from the one place the suite keeps
    them: table_edges.make_policy (linear: tests/test_linear_policy_gpu.py, mlp: tests/test_mlp_policy_gpu.py)"""
    return E.make_policy(ct, "linear" if kind == "linear" else "mlp16", np.zeros(1, np.int64))[2]


def decide(x, live, t, budget_left, logit_fn, ties, uniform=None, require_budget=False, gate=None, schedule=None):
    """One day's decisions on the rows x = cat(obs, f), shared by the stepped twin (twin_loop) and the host walk
    (host_walk). Returns (own: the policy's draw or the schedule's label, act: what is attempted after require_budget
    and the gate, tie: near-tie flags of live envs, gated: live envs on a closed day)."""
    rows = np.arange(len(t))
    z, mag = logit_fn(x)
    if uniform is None:
        own = z > 0
        tie = live & (np.abs(z) <= ties[0] * mag)
    else:
        s = 1.0 / (1.0 + np.exp(-z))
        u = uniform(t).astype(np.float64)
        own = u < s
        tie = live & (np.abs(s - u) <= ties[1])
    if schedule is not None:
        own, tie = schedule[rows, t].copy(), np.zeros(len(t), bool)
    act = own.copy()
    gated = np.zeros(len(t), bool)
    if require_budget:
        act &= budget_left > 0
    if gate is not None:
        gated = live & ~gate[rows, t]
        act &= gate[rows, t]
    return own, (act & live).astype(np.int32), tie, gated


def host_walk(V, ct, tup, spec, logit_fn, n_steps, kind, uniform=None, require_budget=False, gate=None):
    """`a = policy(cat(obs, f)); step(a)` on the vector oracle alone (table_edges.oracle_reset / oracle_step), with
    twin_loop's own decision step. Returns per env: tie, alerts, over, and the bitmaps days / att [N, T]."""
    E.oracle_reset(V, tup)
    n = len(tup["budget"])
    acc = dict(tie=np.zeros(n, bool), alerts=np.zeros(n, np.int64), over=np.zeros(n, np.int64),
               days=np.zeros((n, ct.T), bool), att=np.zeros((n, ct.T), bool))
    ties, rows = tie_bounds(ct, kind), np.arange(n)
    for _ in range(n_steps):
        live = ~V._finished
        if not live.any():
            break
        st = dict(t=V.t.copy(), n_days=tup["n_days"], county_w=tup["county_w"], year_i=tup["year_i"])
        x = np.concatenate([V.obs.astype(np.float32), inputs(ct, spec["feature"], spec["days"], st)], axis=1)
        _, act, tie, _ = decide(x, live, st["t"], V.budget - V.used, logit_fn, ties, uniform, require_budget, gate)
        acc["tie"] |= tie
        atb = V.used == V.budget
        _, _, actual, _ = E.oracle_step(V, act.astype(np.int64))
        acc["alerts"] += np.where(live, actual, 0)
        acc["over"] += live & (act == 1) & atb
        acc["days"][rows[live & (actual == 1)], st["t"][live & (actual == 1)]] = True
        acc["att"][rows[live & (act == 1)], st["t"][live & (act == 1)]] = True
    return acc


def series(ct, feature):
    """f32 [S_w * Y, T]: h along every (county, year) episode."""
    slot = ct.obs_slot[ct.feature_names.index(feature)]
    return np.ascontiguousarray(ct.X[:, :, slot].T.astype(np.float32))


def held_day(t):
    """day of the row the agent holds when it decides about env day t (Q6)"""
    return np.maximum(np.asarray(t, np.int64) - 1, 0)


def inputs(ct, feature, D, st):
    """f32 [N, D] from a host state dict (t, n_days, county_w, year_i)."""
    h = series(ct, feature)
    row = np.asarray(st["county_w"], np.int64) * ct.Y + np.asarray(st["year_i"], np.int64)
    r = held_day(st["t"])
    nd = np.asarray(st["n_days"], np.int64)
    f = np.zeros((len(r), D), np.float32)
    for k in range(1, D + 1):
        ok = r + k < nd
        f[ok, k - 1] = h[row[ok], r[ok] + k] - h[row[ok], r[ok]]  # f32 - f32, one rounding
    return f


def midpoint_threshold(ct, feature, k=1):
    """c halfway (in fp64, returned as the f32 nearest to it) between the two neighbouring distinct values of
    h(d + k) - h(d) around their median: `f_k - c > 0` then has no tie anywhere in the table, and 0 - c < 0"""
    h = series(ct, feature)
    d = np.unique((h[:, k:] - h[:, :-k]).astype(np.float32))
    d = d[d > 0]
    i = len(d) // 2
    c = np.float32(0.5 * (float(d[i]) + float(d[i + 1])))
    assert d[i] < c < d[i + 1]
    return c


def linear_logit(W, b, g, x):
    """fp64 logits of [G, n_obs + D] f32 parameters on the rows x = cat(obs, f), and the near-tie scale sum |products|."""
    prod = x.astype(np.float64) * W.astype(np.float64)[g]
    return prod.sum(axis=1) + b.astype(np.float64)[g], np.abs(prod).sum(axis=1)


def host_state(env):
    return {k: v.cpu().numpy() for k, v in env.state().items()}


def twin_loop(env, ct, spec, logit_fn, n_steps, kind, uniform=None, require_budget=False, gate=None, schedule=None):
    """Step `env` for n_steps days with a = policy(cat(obs, restated f)). logit_fn(x) -> (fp64 logit, near-tie scale).
    kind "linear" / "mlp" picks the near-tie rule; uniform(t) the sampled policy's u; gate: bool [N, T] allowed days.
    schedule: bool [N, T] -- the attempted action is the schedule's bit, not the policy's choice (teacher forcing).
    Returns ret, alerts, over, days, att, tie per env, and the trajectory [S, N(, n_obs + D)]: x (the rows cat(obs, f)
    held before every decision), action (the policy's own draw / the label), valid, reward, alert."""
    import torch

    n, T = env.num_envs, ct.T
    acc = dict(ret=np.zeros(n), alerts=np.zeros(n, np.int64), over=np.zeros(n, np.int64),
               days=np.zeros((n, T), bool), att=np.zeros((n, T), bool), tie=np.zeros(n, bool))
    rows = np.arange(n)
    D = spec["days"]
    ties = tie_bounds(ct, kind)
    tr = dict(x=np.zeros((n_steps, n, ct.n_obs + D), np.float32), action=np.zeros((n_steps, n), np.int64),
              valid=np.zeros((n_steps, n), bool), reward=np.zeros((n_steps, n), np.float32),
              alert=np.zeros((n_steps, n), bool), gated=np.zeros((n_steps, n), bool))
    acc["traj"] = tr
    # step() takes the whole batch, so envs whose (ragged) episode is over go on being stepped with action 0, which
    # moves their 14-day window and last_actual: every env's state and row are kept as its own last live step left them
    prev_live, final, final_obs = np.ones(n, bool), None, None

    def keep(st, obs):
        nonlocal final, final_obs
        if final is None:
            final, final_obs = {k: v.copy() for k, v in st.items()}, obs.copy()
        for k in final:
            final[k][prev_live] = st[k][prev_live]
        final_obs[prev_live] = obs[prev_live]

    for s_ in range(n_steps):
        st = host_state(env)
        obs_now = env._obs.cpu().numpy()
        keep(st, obs_now)
        live = st["finished"] == 0
        prev_live = live
        if not live.any():
            break
        x = np.concatenate([obs_now, inputs(ct, spec["feature"], spec["days"], st)], axis=1)
        own, act, tie, gated = decide(x, live, st["t"], st["budget"] - st["used"], logit_fn, ties, uniform,
                                      require_budget, gate, schedule)
        acc["tie"] |= tie
        tr["x"][s_], tr["action"][s_], tr["valid"][s_], tr["gated"][s_] = x, own, live, gated
        atb = st["used"] == st["budget"]
        actual = act.astype(bool) & ~atb
        _, r, _, _, _ = env.step(torch.as_tensor(act, device=env.device))
        tr["reward"][s_], tr["alert"][s_] = r.cpu().numpy(), live & actual
        acc["ret"] += np.where(live, r.cpu().numpy().astype(np.float64), 0.0)
        acc["alerts"] += live & actual
        acc["over"] += live & (act == 1) & atb
        acc["days"][rows[live & actual], st["t"][live & actual]] = True
        acc["att"][rows[live & (act == 1)], st["t"][live & (act == 1)]] = True
    keep(host_state(env), env._obs.cpu().numpy())
    acc["state"], acc["obs"] = final, final_obs
    return acc


def policy_uniform(seed, gid0, st0):
    """u of (seed, global env id, episode number, day), as rollout(sample=True) draws it; st0: a state with
    "episode_no" (0 for every env after the first reset)"""
    n = len(st0["episode_no"])
    return lambda t: O.devrng_policy_uniform_vec(seed, gid0 + np.arange(n), st0["episode_no"], t)


def widen_linear(ct, W, D, seed, scale=0.5):
    """[G, n_obs] -> [G, n_obs + D]: D lookahead columns appended, k = 1 first"""
    rng = np.random.default_rng(seed)
    return np.concatenate([W, (rng.standard_normal((W.shape[0], D)) * scale).astype(np.float32)], axis=1)


def widen_net(layers, D, seed, scale=0.5):
    """the nets of tests/policy_gradient_mlp_cases.py with D more input columns on the first layer"""
    rng = np.random.default_rng(seed)
    W1, b1 = layers[0]
    extra = (rng.standard_normal(W1.shape[:-1] + (D,)) * scale).astype(np.float32)
    return [(np.concatenate([W1, extra], axis=-1), b1)] + list(layers[1:])
