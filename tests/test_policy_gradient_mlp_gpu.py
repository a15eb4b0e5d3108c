"""rollout(mlp, policy_gradient=...) (k_pgm_pass1 / k_pgm_pass2 / k_pgm_reduce, w2a_policy_gradient_mlp) against the fp64
restatement (tests/policy_gradient_mlp_restatement.py), fed as in tests/test_policy_gradient_gpu.py by references that
never touch the kernels under test: the recorded trajectory of an identical twin (B, rollout(record=True)), the rewards
of a twin stepped with no alerts (C), and on the synthetic table the vector oracle stepped with B's recorded actions.
Every comparison requires |g - g_ref| <= bound for every parameter and prints the largest ratio (the bound and its
derivation: the restatement's docstring).

Which code runs: the nets of NETS reach <16, 1> and <64, 2> only. test_gradient_every_instantiation runs the matrix of
tests/policy_gradient_mlp_cases.py, all six (WIDTH, LAYERS) pairs of k_pgm_pass1 / k_pgm_pass2 with padded units under
both activations; test_gradient_tile_counts runs 2 and 16 tiles per wave of pass 2 and k_pgm_scan with two chunks per
thread; test_non_group_major_order_gives_nan holds the NaN contract of include/w2a.h through the C entry point."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from policy_gradient_mlp_cases import MATRIX, net as _case_net  # noqa: E402
from policy_gradient_mlp_restatement import policy_gradient_mlp_fp64  # noqa: E402
from policy_gradient_restatement import forced_days  # noqa: E402
from test_policy_gradient_gpu import _equal, _never, _npd, _oracle_replay  # noqa: E402

from oracle import heatalert_oracle as O  # noqa: E402
from weather2alert_amd import _ffi, policy, synth, tables  # noqa: E402

pytestmark = pytest.mark.gpu

BASELINES = ("none", "no_alert")
SEED = 11
NETS = {"tanh16": ((16,), "tanh", 1), "relu24x40": ((24, 40), "relu", 2), "tanh64x64": ((64, 64), "tanh", 2)}
ALL_NETS = {**NETS, **{name: spec[1:] for name, spec in MATRIX.items()}}
SPANS = {"whole": (0, None), "n17": (0, 17), "mid": (9, 40)}
MATRIX_SPANS = ("whole", "mid")
WORST = {"ratio": 0.0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=6, seed=17, extra_confounder_fips=3)


@pytest.fixture(scope="module")
def ct(sd):
    return tables.compile_from_synth(sd)


@pytest.fixture(scope="module")
def tabs():
    return E.make_tables()


def _net(ct, name, G):
    hidden, act, n_out = ALL_NETS[name]
    layers = [(W[:G], b[:G]) for W, b in _case_net(ct, name, hidden, n_out)]
    return layers, act


def _instantiation(name):
    """'<WIDTH, LAYERS>' of the kernels a net runs, by the host's own padding rule"""
    hidden = ALL_NETS[name][0]
    return f"<{policy.mlp_width(hidden)}, {len(hidden)}>"


def _align256(v):
    return (v + 255) // 256 * 256


def _pgm_layout(n, n_steps, G, width, n_layers):
    """pgm_layout of csrc/w2a_kernels.hip restated: (64-env tiles per wave of pass 2, its waves = chunks, partial
    blocks the workspace holds, bytes). A wave gets ceil(n_tiles / 1024) tiles, at most 16."""
    n_tiles = (n + 63) // 64
    tiles = min(16, max(1, (n_tiles + 1023) // 1024))
    chunks = (n_tiles + tiles - 1) // tiles
    capacity = chunks + min(G, n)
    stride, days = policy.mlp_stride(width, n_layers), n * n_steps
    sizes = (8 * days, days, 8 * n, 4 * n, 4 * chunks, 4 * (chunks + 1), 4 * capacity, 4 * capacity, 8 * capacity * stride)
    return tiles, chunks, capacity, sum(_align256(v) for v in sizes)


def _tiles_line(what, n, n_steps, G, name):
    """prints the tile and chunk counts of a case and holds the restated layout to the library's workspace size, so that
    the counts printed are the ones the kernels run with"""
    hidden = ALL_NETS[name][0]
    width, nl = policy.mlp_width(hidden), len(hidden)
    tiles, chunks, capacity, nbytes = _pgm_layout(n, n_steps, G, width, nl)
    assert _ffi.load().w2a_policy_gradient_mlp_workspace_bytes(n, n_steps, G, width, nl) == nbytes
    print(f"{what}: {n} envs = {(n + 63) // 64} tiles, {tiles} tile(s) per wave of pass 2, {chunks} chunks, "
          f"{capacity} partial blocks, workspace {nbytes / 2**20:.1f} MiB")
    return tiles, chunks


def _policy(ct, name, G, g, require_budget=False, seed=SEED):
    layers, act = _net(ct, name, G)
    pol = dict(kind="mlp", layers=layers, activation=act, sample=True, seed=seed, require_budget=require_budget)
    if G > 1:
        pol["group"] = g
    return pol


def _layers(out):
    got = out["policy_gradient"]["layers"]
    assert all(dW.dtype == torch.float32 and db.dtype == torch.float32 for dW, db in got)
    return [(dW.double().cpu().numpy(), db.double().cpu().numpy()) for dW, db in got]


def _within(got, ref, what, rows=None):
    """every parameter of got within the restatement's bound (rows: the groups to compare); the largest ratio"""
    ratio = 0.0
    for (dW, db), (rW, rb), (bW, bb) in zip(got, ref["layers"], ref["bound"]):
        for x, r, bd in ((dW, rW, bW), (db, rb, bb)):
            if rows is not None:
                x, r, bd = x[rows], r[rows], bd[rows]
            assert x.shape == r.shape, (what, x.shape, r.shape)
            assert np.isfinite(x).all() and np.isfinite(r).all(), what
            diff = np.abs(x - r)
            ratio = max(ratio, float(np.where(bd > 0, diff / np.where(bd > 0, bd, 1.0), 0.0).max()))
            assert (diff <= bd).all(), (what, ratio)
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"{what}: max |g - g_ref| / bound = {ratio:.3e}   (largest so far in this file {WORST['ratio']:.3e})")
    return ratio


def _restate(st0, obs, tr, valid, rew, beta, pol, baseline, g, G):
    forced = forced_days(pol["require_budget"], st0["budget"], st0["used"], tr["alert"], tr["valid"])
    return policy_gradient_mlp_fp64(obs, tr["action"], valid, forced, rew, beta if baseline == "no_alert" else None,
                                    pol["layers"], pol["activation"], g, G)


def _twin_case(make_env, ct, pol, g, G, prefix, n_steps, what):
    """A1 / A2 take the gradient (one per baseline), B records, C is stepped with no alerts -- all from one start.
    Returns (B's start state, the prefix's record, the record, the two gradients)."""
    envs = [make_env() for _ in range(4)]
    A = dict(zip(BASELINES, envs[:2]))
    B, C_ = envs[2], envs[3]
    pre = None
    if prefix:
        for e_ in envs[:2] + [C_]:
            e_.rollout(pol, n_steps=prefix)
        pre = _npd(B.rollout(pol, n_steps=prefix, record=True)["trajectory"])
    st0 = {k: v.cpu().numpy().astype(np.int64) for k, v in B.state().items()}
    tr = _npd(B.rollout(pol, n_steps=n_steps, record=True)["trajectory"])
    trc = _npd(C_.rollout(_never(ct), n_steps=n_steps, record=True)["trajectory"])
    np.testing.assert_array_equal(trc["valid"], tr["valid"])
    assert not trc["alert"].any() and tr["alert"].any() and tr["valid"].any()
    S = tr["valid"].shape[0]
    got = {}
    for bl in BASELINES:
        out = A[bl].rollout(pol, n_steps=n_steps, policy_gradient=bl)
        assert A[bl].check_status() == 0
        # B's recorded actions are the ones the gradient's rollout took (a differing action moves whole terms)
        np.testing.assert_array_equal(out["alerts"].cpu().numpy(), (tr["alert"] & tr["valid"]).sum(axis=0))
        got[bl] = _layers(out)
        ref = _restate(st0, tr["obs"][:S].astype(np.float64), tr, tr["valid"], tr["reward"], trc["reward"], pol, bl, g, G)
        _within(got[bl], ref, f"{what} twin {bl}")
    assert max(np.abs(a - b).max() for (a, _), (b, _) in zip(got["none"], got["no_alert"])) > 0  # the baseline is in
    for e_ in envs:
        e_.close()
    return st0, pre, tr, got


def _twin_and_oracle(dev, sd, ct, net, G, require_budget, span):
    """200 envs from one reset: the recorded twin (both baselines), then every float recomputed in fp64 by the vector
    oracle stepped with the twin's recorded actions. The returned shapes are the policy's own, [G, out, in]."""
    from weather2alert_amd import HeatAlertVecEnv

    n = 200
    g = E.groups(n) if G > 1 else None
    pol = _policy(ct, net, G, g, require_budget)
    prefix, n_steps = SPANS[span]

    def make_env():
        env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=100, similar_climate_counties=True)
        env.reset(seed=5, options={"budget": 10})
        return env

    probe = make_env()
    st_reset = {k: v.cpu().numpy().astype(np.int64) for k, v in probe.state().items()}
    probe.close()
    what = f"{_instantiation(net)} {net} G={G} rb={require_budget} {span}"
    st0, pre, tr, got = _twin_case(make_env, ct, pol, g, G, prefix, n_steps, what)
    for bl in BASELINES:
        assert [(dW.shape, db.shape) for dW, db in got[bl]] == [(W.shape, b.shape) for W, b in pol["layers"]], what
    S = tr["valid"].shape[0]
    V = O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years)
    obs, rew, valid = _oracle_replay(V, st_reset, pre, tr["action"], S)
    _, beta, valid0 = _oracle_replay(V, st_reset, pre, None, S)
    np.testing.assert_array_equal(valid, tr["valid"])
    np.testing.assert_array_equal(valid0, tr["valid"])
    np.testing.assert_array_equal(obs[valid].astype(np.float32), tr["obs"][:S][valid])
    for bl in BASELINES:
        _within(got[bl], _restate(st0, obs, tr, valid, rew, beta, pol, bl, g, G), f"{what} fp64 {bl}")


@pytest.mark.parametrize("span", list(SPANS))
@pytest.mark.parametrize("require_budget", [False, True])
@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("net", list(NETS))
def test_gradient_against_recorded_twin_and_oracle(dev, sd, ct, net, G, require_budget, span):
    """200 envs (no multiple of 64), one- and two-row outputs, G = 1 and 5 interleaved groups, both baselines,
    require_budget on and off, whole episode / 17 days / mid-episode after a 9-day prefix: against the recorded twin, and
    with every float recomputed in fp64 by the vector oracle stepped with the twin's recorded actions."""
    _twin_and_oracle(dev, sd, ct, net, G, require_budget, span)


@pytest.mark.parametrize("span", MATRIX_SPANS)
@pytest.mark.parametrize("net", list(MATRIX))
def test_gradient_every_instantiation(dev, sd, ct, net, span):
    """All six <WIDTH, LAYERS> instantiations of k_pgm_pass1 / k_pgm_pass2, each with a tanh and a ReLU net and with both
    output forms under every padded width (tests/policy_gradient_mlp_cases.py): the doubled accumulators of <16, 2>, the
    two passes per tile and the pitch of 48 of width 32, the one-layer aliasing of the transposed buffers at width 64.
    The tanh nets with padded units ((1,), (7, 13), (17,), (29, 9), (64, 33)) are the ones where a padded unit has
    act' = 1 and only the zero padding of w_out / W2 keeps it out of the gradient. 200 envs, G = 5 interleaved groups,
    whole episode and mid-episode after a 9-day prefix, require_budget alternating over nets and spans; checks as
    test_gradient_against_recorded_twin_and_oracle. The net must pad to the pair it is listed under."""
    pair, hidden, _, _ = MATRIX[net]
    assert (policy.mlp_width(hidden), len(hidden)) == pair
    require_budget = (list(MATRIX).index(net) + MATRIX_SPANS.index(span)) % 2 == 1
    _twin_and_oracle(dev, sd, ct, net, E.G, require_budget, span)


@pytest.mark.parametrize("name", ["ragged", "slot27", "ragged27"])
def test_gradient_on_table_edges(dev, tabs, name):
    """The three tables of tests/table_edges.py with that file's batches and groups (ragged episode lengths down to 1 day
    inside one wave, slot-27 coefficient rows), whole episodes and a mid-episode start after alerts: on the slot-27
    tables the no-alert fork then has to use the decayed 14-day window of the start state."""
    from weather2alert_amd import HeatAlertVecEnv

    tb = tabs[name]
    ct, n = tb.ct, E.N_ENVS[name]
    g = E.groups(n)

    def make_env():
        env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=E.GID0,
                              similar_climate_counties=True)
        env.reset(seed=E.RESET[name]["seed"], options=dict(E.RESET[name]["opts"]))
        return env

    cases = [(False, "relu24x40"), (True, "tanh16")]
    if name == "ragged27":  # and a tanh net of <32, 2> and one of <64, 1>
        cases += [(False, "tanh29x9"), (True, "tanh64_o2")]
    for rb, net in cases:
        pol = _policy(ct, net, E.G, g, rb, seed=E.POLICY_SEED)
        for span, (prefix, n_steps) in (("whole", (0, None)), ("mid", (9, 30))):
            st0, _, tr, _ = _twin_case(make_env, ct, pol, g, E.G, prefix, n_steps,
                                       f"{name} {_instantiation(net)} {net} rb={rb} {span}")
            if span == "mid":  # alerts inside the 14-day window of the start state
                assert ((st0["hist14"] != 0) & (st0["finished"] == 0)).any()


@pytest.mark.parametrize("mode", ["disabled", "lockstep_same_step", "order"])
def test_gradient_changes_nothing_else(dev, ct, mode):
    """With and without the keyword, identical twins: every other key, the observation buffer, state() and final_return
    bit-identical (alert_mask, posterior_returns and hindsight on), also with a user-supplied "order"; two identical
    gradient calls are bit-identical."""
    from weather2alert_amd import HeatAlertVecEnv

    n, G = 3000 + 7, 3
    kw = dict(tables=ct, device=dev)
    if mode != "lockstep_same_step":
        kw.update(autoreset="disabled")
    envs = [HeatAlertVecEnv(n, **kw) for _ in range(3)]
    for e_ in envs:
        e_.reset(seed=4, options={"budget": 5})
    A, A2, B = envs
    g = np.random.default_rng(5).integers(0, G, n)
    pol = _policy(ct, "relu24x40", G, g, require_budget=True, seed=2)
    if mode == "order":
        pol["order"] = np.random.default_rng(6).permutation(n)
    for steps in (37, None, None):
        extra = dict(alert_mask=True, posterior_returns=True, hindsight=True)
        oa = A.rollout(pol, n_steps=steps, policy_gradient=True, **extra)
        oa2 = A2.rollout(pol, n_steps=steps, policy_gradient="no_alert", **extra)
        ob = B.rollout(pol, n_steps=steps, **extra)
        assert set(oa) - set(ob) == {"policy_gradient"} and not [k for k in oa if k.startswith("_")]
        for k, v in ob.items():
            _equal(oa[k], v, k)
        for (dW, db), (dW2, db2) in zip(oa["policy_gradient"]["layers"], oa2["policy_gradient"]["layers"]):
            _equal(dW, dW2, "dW")
            _equal(db, db2, "db")
        sa, sb = A.state(), B.state()
        for k in sb:
            assert torch.equal(sa[k], sb[k]), k
        assert torch.equal(A._obs, B._obs) and torch.equal(A._final_return, B._final_return)
        assert A.check_status() == 0 and B.check_status() == 0
    for e_ in envs:
        e_.close()


def test_gradient_group_layout_and_flush(dev, ct):
    """Group sizes 70 / 5 / 125 and an empty fourth group: the second wave of the group-major order spans three groups
    (the flush on a group change), the empty group gives NaN. Permuted labels and added envs of other groups leave a
    group's gradient inside the bound."""
    from weather2alert_amd import HeatAlertVecEnv

    n, G = 200, 4
    g = np.concatenate([np.zeros(70, np.int64), np.full(5, 1), np.full(125, 2)])
    g = g[np.random.default_rng(2).permutation(n)]
    layers, act = _net(ct, "tanh64x64", G)

    def mlp(layers_, g_):
        return dict(kind="mlp", layers=layers_, activation=act, group=g_, sample=True, seed=SEED, require_budget=False)

    def run(n_, pol_, **kw):
        env = HeatAlertVecEnv(n_, tables=ct, device=dev, autoreset="disabled", env_gid0=100, similar_climate_counties=True)
        env.reset(seed=5, options={"budget": 6})
        st0 = {k: v.cpu().numpy().astype(np.int64) for k, v in env.state().items()}
        out = env.rollout(pol_, **kw)
        env.close()
        return out, st0

    pol = mlp(layers, g)
    out, st0 = run(n, pol, policy_gradient="no_alert")
    raw = _layers(out)
    assert all(np.isnan(dW[3]).all() and np.isnan(db[3]).all() for dW, db in raw)  # a group without envs
    tr = _npd(run(n, pol, record=True)[0]["trajectory"])
    beta = _npd(run(n, _never(ct), record=True)[0]["trajectory"])
    assert not beta["alert"].any()
    S = tr["valid"].shape[0]
    ref = _restate(st0, tr["obs"][:S].astype(np.float64), tr, tr["valid"], tr["reward"], beta["reward"], pol, "no_alert", g, G)
    _within(raw, ref, "flush 70/5/125", rows=[0, 1, 2])
    perm = np.array([2, 0, 3, 1])  # new label of old group k
    pl = [(np.empty_like(W), np.empty_like(b)) for W, b in layers]
    for (Wp, bp), (W, b) in zip(pl, layers):
        Wp[perm], bp[perm] = W, b
    permuted = [(dW[perm], db[perm]) for dW, db in _layers(run(n, mlp(pl, perm[g]), policy_gradient="no_alert")[0])]
    _within(permuted, ref, "labels permuted", rows=[0, 1, 2])
    g2 = np.concatenate([g, 1 + np.arange(300) % 3])  # 300 more envs join groups 1..3; group 0 keeps its envs and ids
    bigger = _layers(run(n + 300, mlp(layers, g2), policy_gradient="no_alert")[0])
    _within(bigger, ref, "other groups grown", rows=[0])


def _consecutive_groups_case(dev, sd, ct, n, per, net, reset_seed, scale_seed, ks, what):
    """n envs in groups of `per` consecutive env ids (the order is then the identity and group-major), the parameters of
    group 0 of `net` scaled per group, one whole episode with the no-alert baseline: finite everywhere and every env
    done; the groups `ks` rebuilt as small batches with the same global env ids, recorded, replayed by the oracle, lie
    inside the bound. Returns (tiles per wave of pass 2, chunks)."""
    from weather2alert_amd import HeatAlertVecEnv

    G = (n + per - 1) // per
    g = np.arange(n) // per
    act = ALL_NETS[net][1]
    rng = np.random.default_rng(scale_seed)
    l1, _ = _net(ct, net, 1)
    layers = [(np.repeat(W, G, axis=0) * rng.uniform(0.5, 1.5, (G, 1, 1)).astype(np.float32),
               np.repeat(b, G, axis=0) * rng.uniform(0.5, 1.5, (G, 1)).astype(np.float32)) for W, b in l1]
    layout = _tiles_line(f"{what} {_instantiation(net)} {net}", n, ct.T, G, net)
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", similar_climate_counties=True)
    env.reset(seed=reset_seed)
    out = env.rollout(dict(kind="mlp", layers=layers, activation=act, group=g, sample=True, seed=SEED),
                      policy_gradient="no_alert")
    assert env.check_status() == 0 and out["done"].all()
    got = _layers(out)
    assert all(np.isfinite(dW).all() and np.isfinite(db).all() for dW, db in got)
    env.close()
    V = O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years)
    for k in ks:
        nk = min(per, n - k * per)
        polk = dict(kind="mlp", layers=[(W[k:k + 1], b[k:k + 1]) for W, b in layers], activation=act, sample=True,
                    seed=SEED, require_budget=False)
        B = HeatAlertVecEnv(nk, tables=ct, device=dev, autoreset="disabled", env_gid0=k * per, similar_climate_counties=True)
        B.reset(seed=reset_seed)
        st0 = {kk: v.cpu().numpy().astype(np.int64) for kk, v in B.state().items()}
        tr = _npd(B.rollout(polk, record=True)["trajectory"])
        B.close()
        assert tr["alert"].any() and not tr["action"][tr["valid"]].all()  # the group's policy takes both actions
        S = tr["valid"].shape[0]
        obs, rew, valid = _oracle_replay(V, st0, None, tr["action"], S)
        _, beta, _ = _oracle_replay(V, st0, None, None, S)
        np.testing.assert_array_equal(valid, tr["valid"])
        ref = _restate(st0, obs, tr, valid, rew, beta, polk, "no_alert", None, 1)
        _within([(dW[k:k + 1], db[k:k + 1]) for dW, db in got], ref, f"{what}, group {k} ({nk} envs)")
    return layout


def test_gradient_many_waves(dev, sd, ct):
    """65 536 envs, G = 64 (group = env id // 1024), [16] tanh, one whole episode: partial blocks across workgroups.
    Finite everywhere, and 4 groups rebuilt as small batches with the same global env ids, recorded and replayed by the
    oracle, lie inside the bound."""
    assert _consecutive_groups_case(dev, sd, ct, 1 << 16, 1024, "tanh16", 77, 8, range(5, 64, 16), "many waves")[0] == 1


def test_gradient_several_tiles_per_wave(dev, sd, ct):
    """131 272 envs: above 65 536 a wave of the second pass covers several 64-env tiles (here 3, 192 envs), adds each
    tile's registers into the partial block it already holds, and carries the current group and its env count from tile
    to tile. Groups of 1 000 consecutive env ids, so every group boundary falls inside a tile and most of them inside a
    wave's second or third tile (group 2 starts at slot 80 of its wave, group 3 at 120); the last group has 272 envs.
    Finite everywhere, and four groups rebuilt as small batches with the same global env ids lie inside the bound."""
    n = (1 << 17) + 200
    G = (n + 999) // 1000
    assert _consecutive_groups_case(dev, sd, ct, n, 1000, "tanh16", 78, 9, (2, 3, 70, G - 1),
                                    "several tiles per wave")[0] == 3


@pytest.fixture(scope="module")
def short():
    """a 12-day table, so that a million envs take seconds"""
    sd = synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=6, n_days=12, seed=23, extra_confounder_fips=3)
    return sd, tables.compile_from_synth(sd)


@pytest.mark.parametrize("n,tiles,chunks", [(65_736, 2, 514), (1_048_969, 16, 1025)])
def test_gradient_tile_counts(dev, short, n, tiles, chunks):
    """The tile counts the other tests do not reach, on a 12-day table, [7, 13] tanh (<16, 2>, padded units), groups of
    1 000 consecutive env ids (group k starts at slot 40 k mod 64 of its tile), groups 0, 1, G // 2 and G - 1 checked as
    in test_gradient_several_tiles_per_wave.
      65 736 envs      1 028 tiles, 2 per wave (128 envs), 514 chunks, G = 66. Group 0: tiles 0..15, chunks 0..7.
                       Group 1 starts at slot 40 of tile 15, the second tile of chunk 7. Group 33: envs 33 000.., from
                       slot 40 of tile 515, the second tile of chunk 257. Group 65, the last: 736 envs, from slot 40 of
                       tile 1 015 (chunk 507) to the 8 envs of tile 1 027 (chunk 513).
      1 048 969 envs   16 391 tiles: the cap of 16 per wave (1 024 envs), 1 025 chunks, G = 1 049 -- k_pgm_scan's 1 024
                       threads then own two chunks each (seg = 2) and its second loop has to advance by the first chunk's
                       count. Group 0: chunk 0, tiles 0..15. Group 1: from slot 40 of tile 15 of chunk 0 to tile 15 of
                       chunk 1, an odd chunk: the second of its thread. Group 524: from slot 32 of tile 11 of chunk 511
                       to tile 11 of chunk 512. Group 1 048, the last: 969 envs, from slot 0 of tile 7 of chunk 1 023 to
                       the 9 envs of tile 6 of chunk 1 024 -- the first group of chunk 1 024, the only chunk of thread 512.
    Pass 1's scratch of the large case is 113 MB (9 B per env-day); the case prints its workspace size."""
    sd, ct = short
    assert ct.T == 12
    G = (n + 999) // 1000
    got = _consecutive_groups_case(dev, sd, ct, n, 1000, "tanh7x13", 79, 10, (0, 1, G // 2, G - 1), f"{tiles} tiles per wave")
    assert got == (tiles, chunks)


def _abi_gradient(env, a, order, baseline, n_steps, tail_blocks):
    """w2a_policy_gradient_mlp through the C ABI on a workspace with `tail_blocks` partial blocks of room behind it, the
    whole buffer filled with 0xA5 first, the true workspace size passed: (return code, grad f32 [G, stride], whether the
    tail still holds the pattern)."""
    lib, dev = env._lib, env.device
    stride = policy.mlp_stride(a.width, a.n_layers)
    wsb = lib.w2a_policy_gradient_mlp_workspace_bytes(env.num_envs, n_steps, a.n_groups, a.width, a.n_layers)
    assert wsb == _pgm_layout(env.num_envs, n_steps, a.n_groups, a.width, a.n_layers)[3]
    buf = torch.full((wsb + tail_blocks * stride * 8 + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    grad = torch.zeros((a.n_groups, stride), dtype=torch.float32, device=dev)
    mp = _ffi.MlpPolicy()
    mp.params, mp.group, mp.order = a.params.data_ptr(), a.group.data_ptr(), order.data_ptr()
    mp.n_groups, mp.n_layers, mp.width, mp.activation = a.n_groups, a.n_layers, a.width, _ffi.MLP_ACTIVATIONS[a.activation]
    mp.sample, mp.require_budget, mp.seed = 1, int(a.require_budget), a.seed
    with torch.cuda.device(dev):
        rc = lib.w2a_policy_gradient_mlp(env._h, C.byref(mp), _ffi.PG_BASELINES[baseline], n_steps, env._obs.data_ptr(),
                                         grad.data_ptr(), buf.data_ptr(), wsb, env._stream())
        torch.cuda.synchronize()
    return rc, grad, bool((buf[wsb:] == 0xA5).all())


def test_non_group_major_order_gives_nan(dev, ct):
    """include/w2a.h: an order that changes group more often than the workspace has partial blocks gives a gradient of
    NaN and no write past the workspace. Only a C caller can pass one (the Python host always passes a group-major
    order). 200 envs = 4 tiles, one per wave, group = env id mod 4 and the identity order: every tile holds four groups,
    16 blocks are wanted, the workspace holds 4 + 4. The buffer has room for all 16 blocks (and more) behind the size that
    is passed, so a broken guard would write into memory this test owns and the pattern there would show it.
    Then group_order(group) on a fresh env from the same reset: finite and inside the bound of the recorded twin."""
    from weather2alert_amd import HeatAlertVecEnv

    n, G, net = 200, 4, "tanh7x13"
    g = np.arange(n) % G
    pol = _policy(ct, net, G, g)

    def make_env():
        env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=100, similar_climate_counties=True)
        env.reset(seed=5, options={"budget": 10})
        return env

    A, A2, B, R, N = (make_env() for _ in range(5))
    a = policy.check_mlp_policy(pol, ct.n_obs, n, ct.obs_slot, dev)
    n_tiles = (n + 63) // 64
    tiles, chunks, capacity, _ = _pgm_layout(n, ct.T, G, a.width, a.n_layers)
    assert (tiles, chunks, capacity) == (1, 4, 8) and n_tiles * G == 16 > capacity
    identity = torch.arange(n, dtype=torch.int32, device=dev)
    rc, grad, tail_ok = _abi_gradient(A, a, identity, "no_alert", ct.T, n_tiles * G)
    assert rc == 0, A._lib.w2a_last_error()
    assert bool(torch.isnan(grad).all())
    assert tail_ok
    assert A.check_status() == 0
    oa, ob = A.rollout(pol), B.rollout(pol)  # the call wrote no state and no observation row
    assert set(oa) == set(ob)
    for k, v in ob.items():
        _equal(oa[k], v, k)
    sa, sb = A.state(), B.state()
    for k in sb:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(A._obs, B._obs) and A.check_status() == 0
    # the same call with the group-major order
    assert a.group_major
    rc, grad, tail_ok = _abi_gradient(A2, a, a.order, "no_alert", ct.T, n_tiles * G)
    assert rc == 0 and tail_ok and A2.check_status() == 0
    got = [(dW.double().cpu().numpy(), db.double().cpu().numpy())
           for dW, db in policy.unpack_mlp_grad(grad, ct.obs_slot, ct.n_obs, a.hidden, a.n_out)]
    st0 = {k: v.cpu().numpy().astype(np.int64) for k, v in R.state().items()}
    tr = _npd(R.rollout(pol, record=True)["trajectory"])
    beta = _npd(N.rollout(_never(ct), record=True)["trajectory"])
    assert tr["alert"].any() and not beta["alert"].any()
    S = tr["valid"].shape[0]
    ref = _restate(st0, tr["obs"][:S].astype(np.float64), tr, tr["valid"], tr["reward"], beta["reward"], pol, "no_alert", g, G)
    _within(got, ref, f"C entry, group-major order {_instantiation(net)} {net}")
    for e_ in (A, A2, B, R, N):
        e_.close()


def test_gradient_refusals(dev, ct):
    """The refusals come before anything is launched: the env's state is untouched."""
    from weather2alert_amd import HeatAlertVecEnv

    env = HeatAlertVecEnv(300, tables=ct, device=dev, autoreset="disabled")
    env.reset(seed=1)
    before = {k: v.clone() for k, v in env.state().items()}
    mlp = _policy(ct, "tanh16", 1, None)
    for pol, kw in ((dict(mlp, sample=False), dict(policy_gradient=True)), (mlp, dict(policy_gradient="critic")),
                    (mlp, dict(policy_gradient=True, record=True))):
        with pytest.raises(ValueError):
            env.rollout(pol, **kw)
    for k, v in env.state().items():
        assert torch.equal(v, before[k]), k
    assert "policy_gradient" not in env.rollout(mlp, n_steps=3, policy_gradient=False)
    env.close()
    pm = HeatAlertVecEnv(300, tables=ct, device=dev, autoreset="disabled", reward_mode="posterior_mean")
    pm.reset(seed=1)
    with pytest.raises(ValueError):
        pm.rollout(mlp, policy_gradient=True)
    pm.close()
