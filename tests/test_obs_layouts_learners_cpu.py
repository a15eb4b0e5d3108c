"""The references of tests/test_obs_layouts_learners_gpu.py without a GPU (the cases are those of
tests/obs_layout_learner_cases.py): every GPU case, replayed by the NumPy oracle, keeps its ambiguity share under the
restatement's cap and is not trivial; each of the five restatements, fed rows in which a column is read where another
one sits, leaves the bound of the true reference (so a slot / column confusion of any kernel fails the GPU comparison);
and gate_fp32 evaluated with a column's slot is a direct read of the feature table at that slot and the lagging day."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obs_layout_learner_cases as C  # noqa: E402
import obs_layouts as L  # noqa: E402
from alert_gate_restatement import gate_fp32  # noqa: E402
from surrogate_restatement import AMBIGUOUS_CAP  # noqa: E402  (fisher_restatement and q_restatement import this one)

CASES = C.by_id(C.all_cases())


@pytest.fixture(scope="module")
def tabs():
    return C.make_tables()


def _replay(tabs, c):
    """(rows, reference, policy, extras) of a case on the oracle's walk"""
    tb = tabs[c["table"]]
    ct = tb.ct
    pol, target = C.params(ct, c)
    sched = C.schedule(tb, c)
    V = C.oracle_at_start(tb, c)
    allowed = C.gate_mask(tb, c, V)[0] if c["gate"] else None
    R = C.oracle_walk(tb, c, sched, force_rb=C.forces_on_budget(c), allowed=allowed, V=V)
    extra = {}
    if c["entry"] == "surrogate":
        ref0 = C.reference(c, R, C.perturbed(pol))
        extra["lp_old"] = ref0["lp"].astype(np.float32).astype(np.float64)  # what the first call hands back, as f32
        extra["ref0"] = ref0
    if c["entry"] == "fisher":
        extra["vec"] = C.vector(pol)
    ref = C.reference(c, R, pol, target, lp_old=extra.get("lp_old"), vec=extra.get("vec"))
    return R, ref, pol, extra


def _not_trivial(c, R, ref, extra, tb):
    what = c["id"]
    S, n = R["valid"].shape
    assert R["valid"].any() and R["issued"].any() and (R["valid"] & ~R["issued"]).any(), what
    assert (R["count14"][R["valid"]] > 0).any(), what  # the 14-day window is not empty throughout
    if tb.ragged:
        assert (R["valid"].sum(0) < S).any(), what  # episodes that end inside the call (or were over on entry)
    if c["bootstrap"]:
        assert R["alive"].any() and (~R["alive"] & R["valid"][0]).any(), what  # a bootstrap row and ends inside the chunk
    if C.forces_on_budget(c):
        assert (R["forced"] & ~R["closed"]).any(), what
    if c["gate"]:
        assert (R["closed"] & ~(R["left_after"] <= 0)).any() and (R["valid"] & ~R["forced"]).any(), what
    if c["entry"] == "surrogate":
        A = C.advantage(S + 2, n)[:S]
        for sign in (1, -1):  # a clipped and a live scored day for each sign of the advantage
            side = ref["m"] & (sign * A > 0)
            assert (side & ~ref["live"]).any() and (side & ref["live"]).any(), (what, sign)
        assert int(extra["ref0"]["clipped"].sum()) == 0
    if c["entry"] == "fisher":
        assert np.abs(ref["quadratic"]).max() > 0, what
    if c["entry"] == "q":
        d = np.abs(ref["td_error"])[R["valid"]]
        assert (d > 0).any(), what
        if c["loss"] == "huber":
            assert (d > c["huber_delta"]).any() and (d < c["huber_delta"]).any(), (what, float(d.min()), float(d.max()))
        if c["rb"]:
            assert ref["masked"].any() and (ref["has_next"] & ~ref["masked"]).any(), what
        have = ~np.isnan(ref["group_loss"])
        assert list(have) == [True, True, False, True], what  # NaN exactly for group 2
        if tb.slot27:  # scored days of envs with a slot-27 coefficient and alerts in the 14-day window
            a2w = tb.a2w[C.tuples(tb, n)["coef_col"]]
            assert (R["valid"] & (R["count14"] > 0))[:, a2w].any() and a2w.any() and not a2w.all(), what


@pytest.mark.parametrize("cid", list(CASES))
def test_gpu_cases_stay_under_the_ambiguity_cap_and_are_not_trivial(tabs, cid):
    """Every case of the GPU file on the oracle's walk: the restatement's ambiguity share (near ties of the Q heads and of
    the clip edge, ReLU units near a kink) is under its cap, scored days exist, issued and not-issued days both occur,
    Huber errors fall on both sides of delta, masked and unmasked next rows occur under require_budget, clipped and
    unclipped days occur for the surrogate, closed days with budget left occur under a gate."""
    c = CASES[cid]
    R, ref, _, extra = _replay(tabs, c)
    share = C.ambiguity(c, ref)
    print(f"{cid}: ambiguity share {share:.2e}, scored days {int(R['valid'].sum())}")
    assert share <= AMBIGUOUS_CAP, (cid, share)
    if "ref0" in extra:
        assert C.ambiguity(c, extra["ref0"]) <= AMBIGUOUS_CAP, cid
    _not_trivial(c, R, ref, extra, tabs[c["table"]])


def test_the_cases_cover_what_they_are_meant_to():
    cs = C.all_cases()
    assert len(CASES) == len(cs)  # ids are unique
    for entry in ("value", "gae", "surrogate", "fisher", "q"):
        mine = [c for c in cs if c["entry"] == entry and not c["gate"] and c["table"] in C.ALL]
        assert {c["table"] for c in mine} == set(C.ALL)
        assert 0.3 < np.mean([c["order"] for c in mine]) < 0.7  # half the cases on the handle's visiting order
        for name in C.ALL:
            assert len({c["order"] for c in mine if c["table"] == name}) == 2
    q = [c for c in cs if c["entry"] == "q" and c["table"] in C.ALL]
    assert {(c["act"], c["double"]) for c in q} == {(a, d) for a in ("tanh", "relu") for d in (False, True)}
    assert sum(c["target"] for c in q) * 3 == len(q) * 2
    assert all(c["rb"] == (c["kind"] == "h24x20") for c in q)
    from weather2alert_amd import policy

    assert [(policy.mlp_width(C.QC.NETS[k][0]), len(C.QC.NETS[k][0])) for k in C.Q_NETS] == [(16, 1), (32, 2), (64, 2)]
    for ent in ("surrogate", "fisher"):
        rb = [c["rb"] for c in cs if c["entry"] == ent and not c["gate"] and c["table"] in C.ALL]
        assert sum(rb) * 2 == len(rb)


# ------------------------------------------------------------------ sensitivity of the references
SENSITIVE = [("value", "linear"), ("gae", "tanh7x13"), ("surrogate", "tanh64x33_o2"), ("fisher", "linear"), ("q", "h7")]


def confused_pair(ct):
    """two observation columns on different slots that a kernel taking a slot for a column would mix up: a table column
    and the column whose index is that column's slot; on `narrow` (every slot but 0 lies past n_obs) the two run-time
    columns whose slots are in reverse order"""
    c = L.offset_column(ct)
    if c is None:
        return ct.feature_names.index("remaining_budget"), ct.feature_names.index("alert_lag1")
    s = int(ct.obs_slot[c])
    assert s < ct.n_obs and s != c
    return c, s


def _parts(ref):
    """[(value, bound), ...] over the parameter arrays of a restatement's result"""
    if "weight" in ref:
        return [(np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1), ref["bound"])]
    return [(x, b) for wb, bb in zip(ref["layers"], ref["bound"]) for x, b in zip(wb, bb)]


def _outside(other, ref):
    """the largest |other - ref| / bound over the components the reference has"""
    worst = 0.0
    for (x, _), (r, bd) in zip(_parts(other), _parts(ref)):
        have = ~np.isnan(r)
        worst = max(worst, float((np.abs(x - r)[have] / np.maximum(bd[have], 1e-300)).max()))
    return worst


@pytest.mark.parametrize("entry,kind", SENSITIVE)
@pytest.mark.parametrize("name", C.ONE_COLUMN)
def test_a_swapped_column_leaves_the_bound_of_every_restatement(tabs, name, entry, kind):
    """The restatement fed the case's own rows with two columns that sit on different slots swapped -- what parameters
    indexed by slot where they should be indexed by column amount to -- gives a result outside the true reference's
    bound in at least one component; the same holds for the parameters sent through obs_layouts.row32's slot order and
    cut back to n_obs columns where the layout allows that."""
    c = CASES[f"{entry}-{name}-{kind}"]
    ct = tabs[name].ct
    R, ref, pol, extra = _replay(tabs, c)
    target = C.params(ct, c)[1]
    a, b = confused_pair(ct)
    assert ct.obs_slot[a] != ct.obs_slot[b]
    Rm = dict(R, obs=R["obs"].copy())
    Rm["obs"][..., [a, b]] = R["obs"][..., [b, a]]
    assert (Rm["obs"] != R["obs"])[:-1][R["valid"]].any()
    mutant = C.reference(c, Rm, pol, target, lp_old=extra.get("lp_old"), vec=extra.get("vec"))
    assert _outside(ref, ref) == 0.0
    r = _outside(mutant, ref)
    print(f"{name} {entry} {kind}: columns {ct.feature_names[a]} / {ct.feature_names[b]} swapped: {r:.3e} times the bound")
    assert r > 1.0, (name, entry, kind, r)
    if max(ct.obs_slot) < ct.n_obs:  # (permuted: slots 0..28 on 29 columns) the rows in slot order
        x32 = L.row32(ct, R["obs"])[..., :ct.n_obs]
        assert (x32 != R["obs"]).any()
        m2 = C.reference(c, dict(R, obs=x32), pol, target, lp_old=extra.get("lp_old"), vec=extra.get("vec"))
        assert _outside(m2, ref) > 1.0


# ------------------------------------------------------------------ one column alone
@pytest.mark.parametrize("name", C.ONE_COLUMN)
def test_one_column_alone_references(tabs, name):
    """The inputs of the GPU file's test_one_column_alone on the oracle's walk: the column moves the linear value and
    the logit, the references are non-zero in that column -- and, for the record, non-zero far outside their bound in
    the columns whose weight and vector entry are zero: d/dw_j of these losses is sum coefficient_s x_js whatever w_j is,
    so "exactly zero in every column with zero weight and a zero vector" is no property of the operations (the GPU test
    asserts zeros exactly where the reference and its bound are zero), and the first-layer column with the largest norm
    is the one whose observations are largest, not the one that carries the weights."""
    tb = tabs[name]
    ct = tb.ct
    col = C.one_column(ct)
    W, b, vW, vb = C.one_column_params(ct, "fisher", col)
    c = dict(CASES[f"fisher-{name}-linear"])
    R = C.oracle_walk(tb, c, C.schedule(tb, c), force_rb=C.forces_on_budget(c))
    x = R["obs"][:-1][R["valid"]][:, col]
    assert np.ptp(x) * C.column_scale(ct, col) > 0.5, name  # the column moves the value and the logit
    pol = dict(kind="linear", weight=W, bias=b, group=C.groups(c))
    vec = dict(weight=vW, bias=vb)
    others = [j for j in range(ct.n_obs) if j != col]
    ref = C.reference(c, R, pol, vec=vec)
    assert (np.abs(ref["weight"][:, col]) > ref["bound"][:, col]).all()
    assert (np.abs(ref["weight"][:, others]) > ref["bound"][:, others]).any()
    cv = dict(CASES[f"value-{name}-linear"])
    Rv = C.oracle_walk(tb, cv, C.schedule(tb, cv))
    refv = C.reference(cv, Rv, pol)
    assert (np.abs(refv["weight"][:, col]) > refv["bound"][:, col]).all()
    assert (np.abs(refv["weight"][:, others]) > refv["bound"][:, others]).any()
    cq = dict(CASES[f"q-{name}-h7"])
    q, tg = C.params(ct, cq)
    q = dict(q, layers=C.one_column_params(ct, "q", col))
    Rq = C.oracle_walk(tb, cq, C.schedule(tb, cq))
    refq = C.reference(cq, Rq, q, tg)
    assert C.ambiguity(cq, refq) <= AMBIGUOUS_CAP
    dW, bd = refq["layers"][0][0], refq["bound"][0][0]
    have = [0, 1, 3]
    assert (np.abs(dW[have][:, :, col]) > bd[have][:, :, col]).any()
    norms = np.sqrt((dW[have] ** 2).sum(axis=(0, 1)))
    print(f"{name}: column {ct.feature_names[col]}; first-layer |dW| by column " + " ".join(f"{v:.2e}" for v in norms)
          + f"; the largest is {ct.feature_names[int(np.argmax(norms))]}")
    if name == "narrow":  # remaining_budget carries the weights; the 14-day count has the larger rows
        assert ct.feature_names[int(np.argmax(norms))] == "alert_2wks" != ct.feature_names[col]


# ------------------------------------------------------------------ the gate's restatement
@pytest.mark.parametrize("prefix", [0, 5])
@pytest.mark.parametrize("name", C.ALL)
def test_gate_restatement_reads_the_slot_on_the_lagging_day(tabs, name, prefix):
    """gate_fp32 evaluated with a column's SLOT on these layouts is X[max(t - 1, 0), county * Y + year, slot] >= tau on
    every day the env still steps and False elsewhere; evaluated with the column's index it is another mask wherever the
    two differ. At the column's median both open and closed days occur, for a scalar and a per-env threshold."""
    tb = tabs[name]
    ct, n = tb.ct, C.N
    tup = C.tuples(tb, n)
    V = C.oracle_at_start(tb, dict(n=n, prefix=prefix))
    start = C.gate_start(tup, V.t, V._finished)
    row = tup["county_w"] * ct.Y + tup["year_i"]
    X = np.asarray(ct.X, np.float32)
    t = np.arange(ct.T)
    cols = C.gate_columns(ct)
    assert len(cols) == (1 if name == "narrow" else 2)
    for col in cols:
        slot = int(ct.obs_slot[col])
        for tau in C.gate_thresholds(ct, tup, col):
            got = gate_fp32(ct.X, ct.Y, slot, start, tau)
            lag = X[np.maximum(t - 1, 0)][:, row, slot].T  # [n, T]
            steps = (t[None, :] >= V.t[:, None]) & (t[None, :] < tup["n_days"][:, None]) & ~V._finished[:, None]
            want = (lag >= np.broadcast_to(np.asarray(tau, np.float32), (n,))[:, None]) & steps
            np.testing.assert_array_equal(got, want)
            assert got[steps].any() and not got[steps].all(), (name, ct.feature_names[col])
            if slot != col and slot < 24:
                assert (gate_fp32(ct.X, ct.Y, col, start, tau) != got).any(), (name, ct.feature_names[col])
    if name == "n8":
        assert ct.feature_names.index("heat_qi") == 1 and ct.obs_slot[1] == 0
    if prefix and tb.ragged:
        assert V._finished.any()
