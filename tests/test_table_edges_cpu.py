"""The references of tests/test_table_edges_gpu.py on their own (no GPU): the three tables have the edges they claim,
the batches drawn on them put many episode lengths into every wave, and the fp64 oracle loop of every policy meets a
near-tie on fewer than 1 % of the envs while the policy really decides -- so the 1 % the GPU tests allow is a property
of the seeds and weight scales, not of the kernels. And those of tests/test_posterior_mean_edges_gpu.py: the fp64
posterior-mean reward (the draw-mean of the restatement) against the posterior-mean oracle, the host restatement of the
int8 kernels' column flags (the slot-27 fixtures run both of their paths in one launch), and built-in policies that
decide."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from posterior_restatement import posterior_returns_fp64  # noqa: E402


@pytest.fixture(scope="module")
def tabs():
    return E.make_tables()


def test_tables_have_the_edges(tabs):
    for name, tb in tabs.items():
        ct = tb.ct
        nd = np.asarray(ct.n_days)
        W = np.asarray(ct.W).reshape(len(tb.sd.fips_list), ct.n_samples, 2, 32)
        if tb.ragged:
            # compile_from_synth accepts 1, 2 and 3 days: none of the shortest lengths is refused
            assert set(E.SHORTEST) <= set(nd.tolist()) and nd.max() == ct.T and nd.min() == 1
            assert len(np.unique(nd)) > 30 and nd.max() - np.sort(nd)[len(E.SHORTEST)] > 0.7 * ct.T
            assert np.array_equal(tb.oracle().n_days_tab.reshape(-1), nd)
        else:
            assert (nd == ct.T).all()
        if tb.slot27:
            assert (W[tb.a2w][..., 27] != 0).any() and (W[~tb.a2w][..., 27] == 0).all()
            assert float(np.abs(W[tb.big][..., :24]).max()) > 20
        else:
            assert (W[..., 27] == 0).all()


def test_batches_mix_lengths_budgets_and_coefficient_kinds(tabs):
    for name, tb in tabs.items():
        n = E.N_ENVS[name]
        assert n % 64 and n % 256
        tup = E.host_tuples(tb, n)
        g = E.groups(n)
        assert np.mean([len(np.unique(g[i:i + 64])) for i in range(0, n, 64)]) > 4.5
        assert (tup["coef_col"] != tup["county_w"]).any()  # similar_climate_counties=True draws other columns
        if tb.ragged:
            assert E.lengths_per_wave(tup["n_days"]) >= 8, E.lengths_per_wave(tup["n_days"])
            assert set(E.SHORTEST) <= set(tup["n_days"].tolist()) and (tup["n_days"] == tb.ct.T).any()
            assert (tup["budget"] == 0).any() and (tup["budget"] > tup["n_days"].min()).any()
            assert (tup["budget"] > tup["n_days"]).any()  # an env that cannot spend its budget
        if tb.slot27:
            c = tup["coef_col"]
            assert tb.a2w[c].mean() > 0.2 and tb.big[c].mean() > 0.2 and (~tb.a2w & ~tb.big)[c].mean() > 0.2


@pytest.mark.parametrize("name", ["ragged", "slot27", "ragged27"])
@pytest.mark.parametrize("pol", list(E.POLICIES))
def test_oracle_loop_decides_and_rarely_ties(tabs, name, pol):
    tb = tabs[name]
    ct, n = tb.ct, E.N_ENVS[name]
    tup = E.host_tuples(tb, n)
    V = tb.oracle()
    E.oracle_reset(V, tup)
    _, fn, ties = E.make_policy(ct, pol, E.groups(n))
    R = E.oracle_record(V, fn, ct.T, ties, uniform=E.policy_uniform(n) if E.POLICIES[pol][1] else None)
    assert V._finished.all() and (V.t == tup["n_days"] - 1).all()
    assert (R["valid"].sum(0) == tup["n_days"]).all() and (R["terminated"].sum(0) == 1).all()
    assert R["tie"].mean() < 0.01, R["tie"].sum()
    ok = ~R["tie"]
    alerted = R["alerts"][ok] > 0
    assert alerted.mean() > 0.05 and (R["alerts"][ok] < np.minimum(tup["n_days"], tup["budget"])[ok]).any()
    assert (R["att"].sum(1)[ok] < tup["n_days"][ok]).mean() > 0.5  # not an alert attempt on every day
    # attempts at the budget happen (the `attempts_over_budget` path) and zero-budget envs never alert
    assert R["over"].sum() > 0 and (R["alerts"][tup["budget"] == 0] == 0).all()
    # the two fp64 references agree where both speak: the restatement's own-draw column fed the oracle's schedule
    st0 = dict(t=np.zeros(n, np.int64), used=np.zeros(n, np.int64), streak=np.zeros(n, np.int64),
               hist14=np.zeros(n, np.int64), finished=np.zeros(n, np.int64),
               **{k: tup[k] for k in ("budget", "n_days", "county_w", "year_i", "coef_col")})
    pr = posterior_returns_fp64(ct.X, ct.W, ct.n_samples, ct.Y, st0, R["days"], ct.T)
    own = pr[np.arange(n), tup["sample"]]
    known = ~tb.a2w[tup["coef_col"]]
    np.testing.assert_allclose(own[known], R["ret"][known], rtol=1e-9, atol=1e-9)
    if tb.slot27:  # the slot-27 coefficients act: the oracle, which has none, is off where a column has one
        assert np.abs(own - R["ret"])[~known].max() > 1e-4


# ------------------------------------------------------------------ reward_mode="posterior_mean"
@pytest.mark.parametrize("name", ["ragged", "slot27", "ragged27"])
def test_posterior_mean_reference_matches_the_oracle_where_it_knows(tabs, name):
    tb = tabs[name]
    R = E.pm_step_reference(tb, 300)
    live, known = R["live"], R["known"]
    assert np.array_equal(np.isnan(R["reward"]), ~live)  # NaN marks exactly the days an env did not step
    assert (live.sum(0) == R["tup"]["n_days"]).all() and (R["done"].sum(0) == 1).all()
    err = np.abs(np.where(live, R["reward"], 0.0) - R["oracle"])
    assert err[:, known].max() <= 1e-12, err[:, known].max()
    np.testing.assert_allclose(R["ret"][known], R["oracle"].sum(0)[known], rtol=0, atol=1e-12 * tb.ct.T)
    if tb.slot27:  # the slot-27 coefficients act: the oracle, which has none, is off on those columns
        assert (~known).any() and err[:, ~known].max() > 1e-4
    else:
        assert known.all()
    # the schedule reaches what the fixed-point ranges and the 4-bit field are about: granted, refused, long windows
    assert R["alert_days"].any() and (R["actions"].sum(0) > R["alert_days"].sum(1)).any()


def test_int8_column_flags_mix_both_paths_on_the_slot27_tables(tabs):
    for name, tb in tabs.items():
        tup = E.host_tuples(tb, E.N_ENVS[name])
        flag = E.pi8_flagged_columns(tb.ct, int(tup["budget"].max()))
        assert flag.shape == (tb.ct.S,)
        if not tb.slot27:
            assert not flag.any()
            continue
        assert flag.any() and not flag.all()  # a strict, non-empty subset: one launch runs both paths
        share = flag[tup["coef_col"]].mean()
        assert 0.2 < share < 0.8, share  # envs on both sides
        assert not flag[tb.a2w].any()  # the slot-27 columns stay on the matrix cores, where slot 27's range matters
        assert np.array_equal(flag, tb.big)


@pytest.mark.parametrize("name", ["ragged", "slot27", "ragged27"])
def test_builtin_policies_decide(tabs, name):
    tb = tabs[name]
    ct, n = tb.ct, E.N_ENVS[name]
    tup = E.host_tuples(tb, n)
    V = tb.oracle("posterior_mean")
    granted = refused = absent = False
    for kind, pol in E.builtin_policies(ct).items():
        E.oracle_reset(V, tup)
        R = E.oracle_builtin_rollout(V, E.oracle_policy(ct, pol), ct.T, E.PolicyStream(n))
        assert V._finished.all() and (V.t == tup["n_days"] - 1).all()
        assert (R["days"].sum(1) == R["alerts"]).all() and not (R["days"] & ~R["att"]).any()
        assert ((R["att"] & ~R["days"]).sum(1) == R["over"]).all()
        assert (R["alerts"] <= np.minimum(tup["budget"], tup["n_days"])).all() and (R["alerts"][tup["budget"] == 0] == 0).all()
        assert R["alerts"].sum() > 0
        if kind != "always":  # not an attempt on every day
            assert (R["att"].sum(1) < tup["n_days"]).mean() > 0.5
        if kind != "threshold":  # require_budget: that kind never attempts at the budget
            assert R["over"].sum() > 0
        granted |= bool(R["alerts"].any())
        refused |= bool(R["over"].any())
        absent |= bool((R["att"].sum(1) < tup["n_days"]).any())
    assert granted and refused and absent
