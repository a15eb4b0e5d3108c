"""The references of tests/test_actor_critic_layouts_gpu.py without a GPU (the cases are those of
tests/actor_critic_layout_cases.py): every GPU case, replayed by the NumPy oracle and restated in fp64, keeps its
ambiguity share under the restatement's cap and is not trivial; the case matrix covers what it is meant to; the ragged
batches hold the 1-, 2- and 3-day episodes and full-length ones, stepping from the first call-day of the cases that start
at reset; on the slot-27 tables the restatement fed the oracle's own rewards -- which lack the slot-27 term, as a kernel
whose reward chain skipped that slot would -- leaves the bounds of the true reference; and the host side of the entry
point (policy.check_actor_critic_net, policy.unpack_mlp_heads_grad) puts every first-layer weight and gradient entry on
the slot of its observation column, stated here column by column from the two-head block layout of include/w2a.h."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import actor_critic_layout_cases as K  # noqa: E402
import obs_layout_learner_cases as C  # noqa: E402
import obs_layouts as L  # noqa: E402
from actor_critic_restatement import AMBIGUOUS_CAP  # noqa: E402

from weather2alert_amd import policy  # noqa: E402


@pytest.fixture(scope="module")
def tabs():
    return K.make_tables()


# ------------------------------------------------------------------ 1: the oracle's replay of every case
@pytest.mark.parametrize("cid", list(K.CASES))
def test_gpu_cases_stay_under_the_ambiguity_cap_and_are_not_trivial(tabs, cid):
    """ambiguous_share (days inside the clip edge's error band) + near_kink + near_tie <= AMBIGUOUS_CAP on the oracle's
    walk, and actor_critic_cases.not_trivial: alerts and non-alerts are scored, epoch cases clip some days and not
    others, gated and at-budget cases force days that keep their value term. On the slot-27 tables scored days belong to
    envs with a slot-27 coefficient and alerts in the 14-day window."""
    c = K.CASES[cid]
    tb = tabs[c["table"]]
    R = K.walk(tb, c)
    ref = K.reference(tb, c, R)
    share = K.ambiguity(ref)
    print(f"{cid}: ambiguity share {share:.2e}, scored {int(ref['days'].sum())} of {int(ref['stepped'].sum())} days, "
          f"clipped {int(ref['clipped'].sum())}")
    assert share <= AMBIGUOUS_CAP, (cid, share)
    K.not_trivial(c, R, ref, cid)
    S = R["valid"].shape[0]
    if tb.ragged:
        assert (R["valid"].sum(axis=0) < S).any(), cid  # episodes that end inside the call (or were over on entry)
    if c["bootstrap"]:
        assert R["alive"].any() and (~R["alive"] & R["valid"][0]).any(), cid  # a bootstrap row, and ends inside the chunk
    if c["gate"]:
        assert (R["closed"] & (R["left_after"] > 0)).any(), cid  # closed days with budget left
    if c["rb"]:
        assert (R["forced"] & ~R["closed"]).any(), cid  # days forced by the budget alone
    if tb.slot27:
        a2w = tb.a2w[K.tuples(tb, c["n"])["coef_col"]]
        assert a2w.any() and not a2w.all() and (ref["m"] & (R["count14"] > 0))[:, a2w].any(), cid


def test_the_cases_cover_what_they_are_meant_to():
    """every table in both modes and on both visiting orders; the six instantiations (by the host's own padding rule)
    under both activations, every net with padded units; every ragged table from reset and with a 7-day bootstrap chunk;
    gated cases on permuted and ragged27, at-budget cases on a "sampled" schedule on n28 and slot27; collect on the
    slot-27 tables at the default (gamma, lambda) and at (1, 1); 193 and 300 envs"""
    cs = list(K.CASES.values())
    assert len(cs) == len(K.all_cases())  # ids are unique
    assert set(K.TABLES) == {"permuted", "n28", "n8", "narrow", "permuted_ragged", "n8_ragged", "slot27", "ragged27"}
    assert {(c["table"], c["mode"]) for c in cs} == {(t, m) for t in K.TABLES for m in ("collect", "epoch")}
    for t in K.TABLES:
        assert {c["order"] for c in cs if c["table"] == t} == {False, True}, t
    inst = lambda c: (policy.mlp_width(K.QC.NETS[c["net"]][0]), len(K.QC.NETS[c["net"]][0]))  # noqa: E731
    pairs = {(w, nl) for w in policy.MLP_WIDTHS for nl in (1, 2)}
    assert {(inst(c), c["act"]) for c in cs} == {(p, a) for p in pairs for a in ("tanh", "relu")}
    assert all(any(h != inst(c)[0] for h in K.QC.NETS[c["net"]][0]) for c in cs)
    for t in K.RAGGED:
        mine = [c for c in cs if c["table"] == t]
        assert any(c["prefix"] == 0 and c["n_steps"] is None for c in mine), t
        assert any(c["mode"] == "collect" and c["n_steps"] == 7 and c["bootstrap"] and c["prefix"] == 0 for c in mine), t
    assert {c["table"] for c in cs if c["gate"]} == {"permuted", "ragged27"}
    assert {c["mode"] for c in cs if c["gate"]} == {"collect", "epoch"}
    assert {c["table"] for c in cs if c["rb"] and c["sched"] == "sampled"} == {"n28", "slot27"}
    for t in C.SLOT27:
        settings = {(c["gamma"], c["lam"]) for c in cs if c["table"] == t and c["mode"] == "collect"}
        assert {(K.DEFAULT["gamma"], K.DEFAULT["lam"]), (1.0, 1.0)} <= settings, t
    assert all(c["n"] == (K.N27 if c["table"] in C.SLOT27 else K.N) for c in cs) and (K.N, K.N27) == (193, 300)
    assert all(c["weights"] and c["grouped"] for c in cs) and list(np.unique(K.groups(cs[0]))) == [0, 1, 3]


# ------------------------------------------------------------------ 2: the ragged batches
@pytest.mark.parametrize("table", K.RAGGED)
def test_ragged_batches_hold_the_shortest_and_the_longest_episodes(tabs, table):
    """every ragged batch draws envs on the 1-, 2- or 3-day episodes and envs at the full T; in the cases that start at
    reset both kinds step on the first call-day, and a d-day episode ends on call-day d - 1"""
    tb = tabs[table]
    ct = tb.ct
    n = K.N27 if table in C.SLOT27 else K.N
    assert n < 1000 and n % 64 != 0
    nd = K.tuples(tb, n)["n_days"]
    short, full = nd <= 3, nd == ct.T
    print(f"{table}: {n} envs, {int(short.sum())} on episodes of at most 3 days, {int(full.sum())} at T = {ct.T}")
    assert short.any() and full.any() and nd.min() >= 1
    mine = [c for c in K.CASES.values() if c["table"] == table and c["prefix"] == 0]
    assert len(mine) >= 2
    for c in mine:
        R = K.walk(tb, c)
        S = R["valid"].shape[0]
        assert R["valid"][0].all(), c["id"]
        assert R["valid"][0][short].any() and R["valid"][0][full].any(), c["id"]
        for e in np.nonzero(short)[0]:
            d = int(nd[e])
            assert R["terminal"][d - 1, e] and R["valid"][:, e].sum() == d, (c["id"], e)
        assert (R["valid"][:, full].sum(axis=0) == S).all(), c["id"]
    later = [c for c in K.CASES.values() if c["table"] == table and c["prefix"] > 0]
    for c in later:  # after the prefix those episodes are over on entry
        assert not K.walk(tb, c)["valid"][0][short].any(), c["id"]


# ------------------------------------------------------------------ 3: the slot-27 term is seen
SLOT27_COLLECT = [cid for cid, c in K.CASES.items() if c["table"] in C.SLOT27 and c["mode"] == "collect"]


@pytest.mark.parametrize("cid", SLOT27_COLLECT)
def test_rewards_without_the_slot27_term_leave_the_references_bounds(tabs, cid):
    """The restatement run a second time on the same walk with the oracle's OWN rewards, which have every coefficient but
    the one on slot 27: "return" leaves ret_bound on at least half of the envs whose coefficient column has a slot-27
    coefficient (the others never hold an alert in the 14-day window: no budget, or too few days) and on none of the
    other envs, and the first-layer gradient leaves its bound. So the GPU comparison can see the term."""
    c = K.CASES[cid]
    tb = tabs[c["table"]]
    sched = K.schedule(tb, c)
    R = K.walk(tb, c, sched)
    ref = K.reference(tb, c, R)
    plain = copy.copy(tb)
    plain.slot27 = False  # obs_layout_learner_cases.oracle_walk then keeps the oracle's rewards
    R0 = C.oracle_walk(plain, c, sched, force_rb=c["rb"], allowed=K.gate(tb, c))
    for key in ("obs", "valid", "labels", "forced", "terminal", "issued"):
        np.testing.assert_array_equal(R0[key], R[key])
    mutant = K.reference(tb, c, R0)
    a2w = tb.a2w[K.tuples(tb, c["n"])["coef_col"]]
    outside = np.abs(mutant["ret"] - ref["ret"]) > ref["ret_bound"]
    assert not outside[~a2w].any()
    dW, rW, bW = mutant["layers"][0][0], ref["layers"][0][0], ref["bound"][0][0]
    have = ~np.isnan(rW)
    ratio = float((np.abs(dW - rW)[have] / np.maximum(bW[have], 1e-300)).max())
    print(f"{cid}: without the slot-27 term the return leaves its bound on {int(outside[a2w].sum())} of {int(a2w.sum())} "
          f"envs with the coefficient; first-layer gradient at {ratio:.1f} times its bound")
    assert 2 * int(outside[a2w].sum()) >= int(a2w.sum()) > 0, cid
    assert ratio > 1.0, (cid, ratio)


# ------------------------------------------------------------------ one column alone: the references
@pytest.mark.parametrize("name", K.ONE_COLUMN)
def test_one_column_alone_references(tabs, name):
    """The inputs of the GPU file's test_one_column_alone on the oracle's walk, for the net as built and with the
    column's weights shifted: the column sits off its index and moves the hidden units over its range, the ambiguity
    share stays under the cap, the case stays non-trivial, the reference's first-layer dW is outside its bound of zero in
    that column, exactly zero with a zero bound in every column whose input is 0 on every stepped day (permuted has
    two; n8 and narrow have none), and the shift moves the per-env outputs beyond their bounds."""
    tb = tabs[name]
    ct = tb.ct
    c = K.CASES[K.ONE_COLUMN_CASES[name]]
    col = K.one_column(ct)
    assert ct.obs_slot[col] != col
    R = K.walk(tb, c)
    S = R["valid"].shape[0]
    x = R["obs"][:S][R["valid"]][:, col]
    assert np.ptp(x) * C.column_scale(ct, col) > 0.5, name
    zero = K.zero_columns(R)
    assert col not in zero and len(zero) == (2 if name == "permuted" else 0), (name, zero)
    have = [0, 1, 3]
    refs = []
    for shift in (0.0, K.ONE_COLUMN_SHIFT):
        layers = K.one_column_net(ct, c, col, shift)
        others = [j for j in range(ct.n_obs) if j != col]
        assert not layers[0][0][:, :, others].any() and (layers[0][0][:, :, col] != 0).all()
        ref = K.reference(tb, c, R, layers=layers)
        assert K.ambiguity(ref) <= AMBIGUOUS_CAP, (name, shift, K.ambiguity(ref))
        K.not_trivial(c, R, ref, (name, shift))
        dW, bd = ref["layers"][0][0][have], ref["bound"][0][0][have]
        assert (np.abs(dW[:, :, col]) > bd[:, :, col]).any(), (name, shift)
        assert not dW[:, :, zero].any() and not bd[:, :, zero].any(), (name, shift)
        refs.append(ref)
    a, b = refs
    assert (np.abs(a["vl"] - b["vl"]) > a["vl_bound"] + b["vl_bound"]).any(), name
    assert (np.abs(a["H"] - b["H"]) > a["H_bound"] + b["H_bound"]).any(), name


# ------------------------------------------------------------------ 4: the host's packing
PACKED = ("permuted", "n28", "narrow")


def _block_offsets(w, nl):
    """offsets in a two-head block (include/w2a.h: W2A_MLP_HEADS_STRIDE): W1[32][w], b1[w], (W2[w][w], b2[w]), wo0[w],
    wo1[w], bo0, bo1, 2 pad"""
    off = dict(W1=0, b1=32 * w)
    nxt = 32 * w + w
    if nl == 2:
        off.update(W2=nxt, b2=nxt + w * w)
        nxt += w * w + w
    off.update(wo0=nxt, wo1=nxt + w, bo0=nxt + 2 * w, bo1=nxt + 2 * w + 1, end=nxt + 2 * w + 4)
    return off


def _unweighted(ct, name):
    return [ct.feature_names.index(f) for f in L.schema(name)[2]]


@pytest.mark.parametrize("net", ["h7", "h24x20"])
@pytest.mark.parametrize("name", PACKED)
def test_first_layer_weights_are_packed_by_slot(tabs, name, net):
    """check_actor_critic_net on the CPU: the whole parameter block, rebuilt here entry by entry. Weight (unit u, column
    j) of the first layer sits at [slot(j)][u] -- the unweighted columns (no reward coefficient; permuted has three, n28
    one) on their own slots like any other --, the rows of slots that hold no observation column and the padded units
    are exactly zero, and the output layer keeps row 0 (the logit) before row 1 (the value)."""
    ct = tabs[name].ct
    n = 12
    hidden = K.QC.NETS[net][0]
    w, nl = policy.mlp_width(hidden), len(hidden)
    layers = K.QC.qnet(ct, net, K.G)
    g = np.array([0, 1, 3])[np.arange(n) % 3]
    pol = policy.check_actor_critic_net(dict(kind="mlp", layers=layers, activation="tanh", group=g), ct.n_obs, n, ct.obs_slot,
                                        torch.device("cpu"))
    off = _block_offsets(w, nl)
    assert (pol.width, pol.n_layers, pol.n_groups, pol.n_out) == (w, nl, K.G, 2)
    assert tuple(pol.params.shape) == (K.G, off["end"]) and off["end"] == policy.mlp_heads_stride(w, nl)
    slots = [int(s) for s in ct.obs_slot[:ct.n_obs]]
    assert len(set(slots)) == ct.n_obs and slots != list(range(ct.n_obs))
    assert any(s != j for j, s in enumerate(slots[:-1]))
    want = np.zeros((K.G, off["end"]), np.float32)
    for k in range(K.G):
        for j, s in enumerate(slots):
            for u in range(hidden[0]):
                want[k, off["W1"] + s * w + u] = layers[0][0][k, u, j]
        want[k, off["b1"]:off["b1"] + hidden[0]] = layers[0][1][k]
        if nl == 2:
            for i in range(hidden[0]):
                for u in range(hidden[1]):
                    want[k, off["W2"] + i * w + u] = layers[1][0][k, u, i]
            want[k, off["b2"]:off["b2"] + hidden[1]] = layers[1][1][k]
        want[k, off["wo0"]:off["wo0"] + hidden[-1]] = layers[-1][0][k, 0]
        want[k, off["wo1"]:off["wo1"] + hidden[-1]] = layers[-1][0][k, 1]
        want[k, off["bo0"]], want[k, off["bo1"]] = layers[-1][1][k, 0], layers[-1][1][k, 1]
    got = pol.params.numpy()
    np.testing.assert_array_equal(got, want)
    W1 = got[:, :32 * w].reshape(K.G, 32, w)
    empty = [s for s in range(32) if s not in slots]
    assert len(empty) == 32 - ct.n_obs and not W1[:, empty].any() and not W1[:, :, hidden[0]:].any()
    for j in _unweighted(ct, name):
        assert slots[j] != j and (W1[:, slots[j], :hidden[0]] == layers[0][0][:, :, j]).all() and W1[:, slots[j]].any()
    assert len(_unweighted(ct, name)) == {"permuted": 3, "n28": 1, "narrow": 0}[name]
    if name == "n28":
        assert 28 in empty  # n_obs a multiple of 4, slot 28 empty
    if name == "narrow":  # the run-time slots in reverse order
        rt = [slots[ct.feature_names.index(f)] for f in ("remaining_budget", "alert_streak", "alert_lag1")]
        assert rt == sorted(rt, reverse=True) and min(rt) >= 24
    assert torch.equal(pol.order, policy.group_order(pol.group)) and pol.group_major


@pytest.mark.parametrize("net", ["h7", "h24x20"])
@pytest.mark.parametrize("name", PACKED)
def test_gradient_entries_are_returned_by_slot(tabs, name, net):
    """unpack_mlp_heads_grad on a block whose every float is its own index (a distinct value each): dW1[g, u, j] is the
    float at [slot(j)][u], unweighted columns included; what sits in a slot without an observation column, in a padded
    unit or in the pad comes back nowhere; the output layer's row 0 is wo0 / bo0 and row 1 wo1 / bo1."""
    ct = tabs[name].ct
    hidden = K.QC.NETS[net][0]
    w, nl = policy.mlp_width(hidden), len(hidden)
    off = _block_offsets(w, nl)
    P = (np.arange(K.G * off["end"], dtype=np.float64) + 1.0).reshape(K.G, off["end"])
    layers = [(dW.numpy(), db.numpy()) for dW, db in policy.unpack_mlp_heads_grad(torch.as_tensor(P), ct.obs_slot, ct.n_obs,
                                                                                 hidden)]
    slots = [int(s) for s in ct.obs_slot[:ct.n_obs]]
    assert [x.shape for wb in layers for x in wb] == \
        [s for d_in, d_out in zip((ct.n_obs,) + tuple(hidden), tuple(hidden) + (2,)) for s in ((K.G, d_out, d_in), (K.G, d_out))]
    for k in range(K.G):
        for j, s in enumerate(slots):
            for u in range(hidden[0]):
                assert layers[0][0][k, u, j] == P[k, off["W1"] + s * w + u], (k, u, j)
        np.testing.assert_array_equal(layers[0][1][k], P[k, off["b1"]:off["b1"] + hidden[0]])
        if nl == 2:
            for i in range(hidden[0]):
                for u in range(hidden[1]):
                    assert layers[1][0][k, u, i] == P[k, off["W2"] + i * w + u]
            np.testing.assert_array_equal(layers[1][1][k], P[k, off["b2"]:off["b2"] + hidden[1]])
        np.testing.assert_array_equal(layers[-1][0][k, 0], P[k, off["wo0"]:off["wo0"] + hidden[-1]])
        np.testing.assert_array_equal(layers[-1][0][k, 1], P[k, off["wo1"]:off["wo1"] + hidden[-1]])
        assert layers[-1][1][k, 0] == P[k, off["bo0"]] and layers[-1][1][k, 1] == P[k, off["bo1"]]
    returned = np.concatenate([x.ravel() for wb in layers for x in wb])
    assert len(np.unique(returned)) == len(returned)  # no float of the block comes back twice
    W1 = P[:, :32 * w].reshape(K.G, 32, w)
    empty = [s for s in range(32) if s not in slots]
    dropped = np.concatenate([W1[:, empty].ravel(), W1[:, :, hidden[0]:].ravel(), P[:, off["bo1"] + 1:].ravel()])
    assert len(dropped) > 0 and not np.isin(dropped, returned).any()
    # the identity in place of obs_slot returns other floats wherever a column sits off its index
    ident = policy.unpack_mlp_heads_grad(torch.as_tensor(P), list(range(ct.n_obs)), ct.n_obs, hidden)[0][0].numpy()
    off_index = [j for j, s in enumerate(slots) if s != j]
    assert off_index and (ident[:, :, off_index] != layers[0][0][:, :, off_index]).all()
