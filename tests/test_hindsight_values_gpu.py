"""hindsight_values() (k_hs_along) and imitation_gradient(labels=...) (the LABELS forms of k_imitation_linear and
k_im_pass1) on the GPU. Exact properties first -- along the optimum's own schedule, against hindsight_optimum() on a
twin stepped through step(), chunking, attempts over budget, determinism, no side effects, budget 0, labels equal to the
schedule -- then the fp64 restatement (tests/hindsight_values_restatement.py) and the imitation restatements on the
twin's rows. The cases are those of tests/hindsight_values_cases.py; one twin and one restatement per case, shared."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hindsight_values_cases as K  # noqa: E402
import table_edges as E  # noqa: E402
from hindsight_values_restatement import hindsight_values_fp64  # noqa: E402
from imitation_restatement import imitation_linear_fp64, imitation_mlp_fp64  # noqa: E402
from policy_gradient_mlp_cases import MATRIX, net as case_net  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(t, b) for t in K.TABLES for b in K.BUDGETS]
FLOATS = ("alert_gain", "value", "loss")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tabs():
    return K.load_tables()


def _clone(st):
    return {k: v.clone() for k, v in st.items()}


def _env(dev, tabs, table, budget, start):
    """a fresh env of the case's batch, stepped `start` days with fixed actions (the same for every twin)"""
    from weather2alert_amd import HeatAlertVecEnv

    ct, kw = tabs[table]
    env = HeatAlertVecEnv(K.N, tables=ct, device=dev, autoreset="disabled", env_gid0=E.GID0, **kw)
    env.reset(seed=11, options={"budget": budget})
    acts = torch.as_tensor(K.prefix_actions(K.N, start, seed=budget + 1), device=dev)
    for d in range(start):
        env.step(acts[d] * (env.state()["finished"] == 0).to(torch.int32))
    return env


def _same(a, b):
    """bit equality of two outputs of hindsight_values() (NaN gains included)"""
    for k in a:
        x, y = a[k], b[k]
        if x.is_floating_point():
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k
        else:
            assert torch.equal(x, y), k


def _issued(sched, st0, T):
    """the alerts a schedule of attempts ISSUES from st0 (what posterior_returns() takes): the first budget - used
    attempts from the start day on; days before it are left as they are (never read)"""
    rem = (st0["budget"] - st0["used"]).clamp(min=0).long()
    day = torch.arange(T, device=sched.device)[None, :]
    att = sched & (day >= st0["t"].long()[:, None])
    return (att & (att.long().cumsum(1) <= rem[:, None])) | (sched & ~att)


_BUNDLES = {}


def _bundle(dev, tabs, table, budget):
    """per (start, p): the start state, the schedule, hindsight_values(value, loss) on env A, and what a twin stepped
    through step() along the schedule saw: rewards and liveness per call-day, the state after k days for the chunking
    test, and hindsight_optimum()'s bit of the day at hand on every 7th call-day and the last three"""
    key = (table, budget)
    if key in _BUNDLES:
        return _BUNDLES[key]
    ct = tabs[table][0]
    rows = torch.arange(K.N, device=dev)
    out = []
    for start in K.STARTS:
        A = _env(dev, tabs, table, budget, start)
        st0 = _clone(A.state())
        assert (st0["budget"] == budget).all()
        for p in K.PS:
            sched = torch.as_tensor(K.schedule(K.N, ct.T, p, seed=int(100 * p) + start), device=dev)
            before = A.state_dict()
            obs_before = A._obs.clone()
            hv = A.hindsight_values(sched, value=True, loss=True)
            after = A.state_dict()
            for k in ("state", "obs", "final_return", "reward", "done"):  # no side effects
                assert torch.equal(before[k], after[k]), k
            assert before["host"] == after["host"] and torch.equal(obs_before, A._obs)
            B = _env(dev, tabs, table, budget, start)
            S = ct.T - start
            twin = dict(reward=torch.zeros((ct.T, K.N), dtype=torch.float64, device=dev),
                        live=torch.zeros((ct.T, K.N), dtype=torch.bool, device=dev), states={}, opt=[], attempts_over=0)
            for s in range(S):
                st = B.state()
                live = st["finished"] == 0
                if not bool(live.any()):
                    break
                t = st["t"].long().clamp(max=ct.T - 1)
                if s in K.CHUNKS:
                    twin["states"][s] = _clone(st)
                if s % 7 == 0 or s >= S - 3:
                    bit = B.hindsight_optimum()["alert_days"][rows, t]
                    twin["opt"].append((s, live.clone(), t.clone(), bit))
                a = sched[rows, t] & live
                twin["attempts_over"] += int((a & (st["used"] >= st["budget"])).sum())
                r = B.step(a.to(torch.int32))[1]
                twin["reward"][s] = torch.where(live, r.double(), torch.zeros_like(r.double()))
                twin["live"][s] = live
            B.close()
            out.append(dict(start=start, p=p, st0=st0, sched=sched, hv=hv, twin=twin))
        assert A.check_status() in (0, 4)  # 4: step() past the ragged table's shortest episodes in the prefix
        A.close()
    _BUNDLES[key] = out
    return out


def _fresh(dev, tabs, table, budget):
    return _env(dev, tabs, table, budget, 0)


@pytest.mark.parametrize("table,budget", CASES)
def test_expert_bits_equal_the_optimum_of_a_stepped_twin(dev, tabs, table, budget):
    """On every 7th call-day and the last three, hindsight_optimum() from the twin's state has the same bit for the
    day at hand as "expert_alert_days"; gains are NaN exactly where no alert is possible; losses are not negative and
    +0 exactly where the issued alert is the expert's; days outside the stretch carry no bits."""
    ct = tabs[table][0]
    rows = torch.arange(K.N, device=dev)
    n_bits = 0
    for c in _bundle(dev, tabs, table, budget):
        hv, twin = c["hv"], c["twin"]
        assert len(twin["opt"]) >= 10
        for s, live, t, bit in twin["opt"]:
            mine = hv["expert_alert_days"][rows, t]
            assert torch.equal(mine[live], bit[live]), (c["start"], c["p"], s)
            n_bits += int(bit[live].sum())
        S = hv["alert_gain"].shape[0]
        assert hv["alert_gain"].shape == hv["value"].shape == hv["loss"].shape == (ct.T, K.N)
        live = twin["live"][:S]
        assert torch.isnan(hv["alert_gain"][~live]).all() and (hv["value"][~live] == 0).all()
        assert (hv["loss"] >= 0).all() and (hv["loss"][~live] == 0).all() and (hv["regret"] >= 0).all()
        assert torch.isfinite(hv["value"]).all() and torch.isfinite(hv["regret"]).all()
        t0, nd = c["st0"]["t"].long(), c["st0"]["n_days"].long()
        day = torch.arange(ct.T, device=dev)[None, :]
        inside = (day >= t0[:, None]) & (day < nd[:, None]) & (c["st0"]["finished"] == 0)[:, None]
        assert not (hv["expert_alert_days"] & ~inside).any()
        if budget == 0:  # no alert is ever possible; value[0] is the value of the empty schedule
            assert torch.isnan(hv["alert_gain"]).all() and not hv["expert_alert_days"].any()
            assert (hv["loss"] == 0).all() and (hv["regret"] == 0).all()
            tail = twin["reward"].flip(0).cumsum(0).flip(0)  # fp64 sums of the f32 rewards, as the DP's values
            np.testing.assert_allclose(hv["value"][0].double().cpu().numpy(), tail[0].cpu().numpy(), rtol=2e-7, atol=0)
        else:
            assert twin["attempts_over"] > 0 or c["p"] < 0.5 or budget > 40
    assert n_bits > 0 or budget == 0


@pytest.mark.parametrize("table,budget", CASES)
def test_chunking_over_budget_attempts_and_determinism(dev, tabs, table, budget):
    """Rows s >= k of one call equal, bit for bit, the call from the state the schedule reaches after k days (k = 7: the
    U bin of a budget-40 env changes; k = 100: a budget-200 env moves from the workspace form to the LDS form);
    clearing the attempts that found no budget changes no output bit; two identical calls give identical bits."""
    ct = tabs[table][0]
    A = _fresh(dev, tabs, table, budget)
    moved = False
    for c in _bundle(dev, tabs, table, budget):
        hv, sched, st0 = c["hv"], c["sched"], c["st0"]
        again = A.hindsight_values(sched, start_state=st0, value=True, loss=True)
        _same(hv, again)
        # attempts that found no budget: the schedule with only the alerts ISSUED (walked on the host)
        day = torch.arange(ct.T, device=dev)[None, :]
        _same(hv, A.hindsight_values(_issued(sched, st0, ct.T), start_state=st0, value=True, loss=True))
        for k, stk in c["twin"]["states"].items():
            part = A.hindsight_values(sched, start_state=stk, value=True, loss=True)
            S = ct.T - k
            for f in FLOATS:
                assert torch.equal(hv[f][k:].view(torch.int32), part[f][:S].view(torch.int32)), (f, k, c["start"], c["p"])
            later = day >= (st0["t"].long() + k)[:, None]
            assert torch.equal(hv["expert_alert_days"] & later, part["expert_alert_days"]), k
            if budget == 200 and table == "mini":
                u0 = int((st0["budget"] - st0["used"]).min())
                uk = int(torch.minimum(stk["budget"] - stk["used"], stk["n_days"] - stk["t"]).max())
                moved |= (not K.lds_fits(min(u0, ct.T - c["start"]), ct.T)) and K.lds_fits(uk, ct.T)
            if budget == 40 and k == 7:
                assert bool((stk["used"] > st0["used"]).any())  # U = min(budget - used, H) changed
    assert moved or not (budget == 200 and table == "mini")
    assert A.check_status() == 0
    A.close()


@pytest.mark.parametrize("table,budget", CASES)
@pytest.mark.parametrize("gated", [False, True])
def test_along_the_optimums_own_schedule(dev, tabs, table, budget, gated):
    """hindsight_optimum()["alert_days"], with and without a gate: the expert bits are the schedule, every loss is +0
    and the regret is 0."""
    ct = tabs[table][0]
    for start in K.STARTS:
        A = _env(dev, tabs, table, budget, start)
        gate = torch.as_tensor(K.schedule(K.N, ct.T, 0.5, seed=5), device=dev) if gated else None
        hs = A.hindsight_optimum(allowed_days=gate)
        hv = A.hindsight_values(hs["alert_days"], allowed_days=gate, value=True, loss=True)
        assert torch.equal(hv["expert_alert_days"], hs["alert_days"])
        assert (hv["loss"].view(torch.int32) == 0).all() and (hv["regret"].view(torch.int32) == 0).all()
        assert budget == 0 or bool(hs["alert_days"].any())
        if gated:  # closed days: no gain, no expert bit
            closed = ~gate
            assert not (hv["expert_alert_days"] & closed).any()
            # an attempt on a closed day is 0 before the budget test
            hv2 = A.hindsight_values(hs["alert_days"] | closed, allowed_days=gate, value=True, loss=True)
            _same(hv, hv2)
        A.close()


@pytest.mark.parametrize("table,budget", CASES)
def test_against_the_fp64_restatement(dev, tabs, table, budget):
    """"value" within (H_e - s) DAY_BAR of the restatement (the maximum over schedules of sums that differ by at most a
    bar per day), "alert_gain" and "loss" within twice that; "regret" against hindsight_optimum()["return"] -
    posterior_returns(start, the alerts the schedule issues)[e, sample_e] within the f32 recursive-summation bound 2 (H_e - 1) 2^-24
    sum_d |r_d| of the twin's rewards, and >= 0. The restatement costs 20 ms (budget 200: 150 ms) per env and schedule,
    so it restates every 4th (8th) env; the kernel runs all 193 and the exact tests above read all of them."""
    ct = tabs[table][0]
    envs = list(range(0, K.N, 8 if budget == 200 else 4))
    A = _fresh(dev, tabs, table, budget)
    worst = dict(value=0.0, alert_gain=0.0, loss=0.0, regret=0.0)
    for c in _bundle(dev, tabs, table, budget):
        hv, st0, sched, twin = c["hv"], c["st0"], c["sched"], c["twin"]
        st = {k: st0[k].cpu().numpy().astype(np.int64) for k in K.HS_KEYS}
        ref = hindsight_values_fp64(ct.X, ct.W, ct.n_samples, ct.Y, st, ct.T, sched.cpu().numpy(), envs=envs)
        H = ref["H"][envs]
        left = np.maximum(H[None, :] - np.arange(ct.T)[:, None], 0)  # H_e - s
        for f, key, mult in (("value", "value", 1), ("alert_gain", "gain", 2), ("loss", "loss", 2)):
            got, want = hv[f].double().cpu().numpy()[:, envs], ref[key][:, envs]
            assert (np.isnan(got) == np.isnan(want)).all(), f
            err = np.nan_to_num(np.abs(got - want))
            bound = mult * left * K.DAY_BAR
            worst[f] = max(worst[f], float((err / np.maximum(bound, 1e-300))[left > 0].max(initial=0.0)))
            assert (err <= bound).all(), (f, c["start"], c["p"], float((err - bound).max()))
        hs = A.hindsight_optimum(st0)
        pr = A.posterior_returns(st0, _issued(sched, st0, ct.T)).gather(1, st0["sample"].long()[:, None])[:, 0]
        want = (hs["return"] - pr).double().cpu().numpy()
        got = hv["regret"].double().cpu().numpy()
        Hall = twin["live"].sum(0).cpu().numpy()
        bound = 2.0 * np.maximum(Hall - 1, 0) * 2.0 ** -24 * twin["reward"].abs().sum(0).cpu().numpy()
        err = np.abs(got - want)
        worst["regret"] = max(worst["regret"], float((err / np.maximum(bound, 1e-300))[bound > 0].max(initial=0.0)))
        assert (err <= bound).all(), (c["start"], c["p"], float((err - bound).max()))
        assert (got >= 0).all()
    print(f"{table} budget {budget}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    A.close()


# ------------------------------------------------------------------ imitation_gradient(labels=...)
def _policies(ct, g):
    rng = np.random.default_rng(3)
    W = (rng.standard_normal((E.G, ct.n_obs)) * 0.4).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] *= 0.1
    pols = {"linear": dict(kind="linear", weight=W, bias=(rng.standard_normal(E.G) * 0.5).astype(np.float32), group=g)}
    for net in ("tanh7x13", "relu33"):
        _, hidden, act, n_out = MATRIX[net]
        pols[net] = dict(kind="mlp", layers=case_net(ct, net, hidden, n_out), activation=act, group=g)
    return pols


@pytest.mark.parametrize("table", K.TABLES)
@pytest.mark.parametrize("gated", [False, True])
def test_labels_equal_to_the_schedule_change_nothing(dev, tabs, table, gated):
    """labels=alert_days: every output equals, bit for bit, the call without the key -- the linear kind and two MLP
    shapes, gated and ungated, with and without require_budget."""
    ct = tabs[table][0]
    A = _env(dev, tabs, table, 8, 25)
    sched = torch.as_tensor(K.schedule(K.N, ct.T, 0.5, seed=3), device=dev)
    gate = torch.as_tensor(K.schedule(K.N, ct.T, 0.6, seed=4), device=dev) if gated else None
    w = np.random.default_rng(8).standard_normal(K.N).astype(np.float32)
    for name, pol in _policies(ct, E.groups(K.N)).items():
        for rb in (False, True):
            pol = dict(pol, require_budget=rb, **({"allowed_days": gate} if gated else {}))
            a = A.imitation_gradient(pol, sched, env_weight=w)
            b = A.imitation_gradient(pol, sched, env_weight=w, labels=sched)
            flat = lambda o: ([o["policy_gradient"]["weight"], o["policy_gradient"]["bias"]] if name == "linear" else  # noqa: E731
                              [x for lay in o["policy_gradient"]["layers"] for x in lay]) + \
                [o["log_likelihood"], o["days"], o["group_log_likelihood"]]
            for x, y in zip(flat(a), flat(b)):
                assert torch.equal(x, y) or torch.equal(x.view(torch.int32), y.view(torch.int32)), (name, rb)
            assert int(a["days"].sum()) > 0
    assert A.check_status() in (0, 4)
    A.close()


@pytest.mark.parametrize("table", K.TABLES)
def test_expert_labels_along_the_learners_schedule(dev, tabs, table):
    """The learner's Bernoulli schedule forces the env, hindsight_values()'s expert bits are the labels: within the
    bounds of the imitation restatements evaluated on a stepped twin's rows with action = labels, "days" equal."""
    ct = tabs[table][0]
    rows = torch.arange(K.N, device=dev)
    g = E.groups(K.N)
    for rb in (False, True):
        A, B = _env(dev, tabs, table, 8, 25), _env(dev, tabs, table, 8, 25)
        sched = torch.as_tensor(K.schedule(K.N, ct.T, 0.5, seed=6), device=dev)
        labels = A.hindsight_values(sched)["expert_alert_days"]
        assert bool((labels != sched).any()) and bool(labels.any())
        S = ct.T
        R = dict(obs=np.zeros((S, K.N, ct.n_obs)), labels=np.zeros((S, K.N), bool), valid=np.zeros((S, K.N), bool),
                 forced=np.zeros((S, K.N), bool))
        for s in range(S):
            st = B.state()
            live = st["finished"] == 0
            if not bool(live.any()):
                break
            t = st["t"].long().clamp(max=ct.T - 1)
            forced = ((st["budget"] - st["used"]) <= 0) & live if rb else torch.zeros_like(live)
            R["obs"][s], R["valid"][s], R["forced"][s] = B._obs.double().cpu().numpy(), live.cpu().numpy(), forced.cpu().numpy()
            R["labels"][s] = (labels[rows, t] & live).cpu().numpy()
            B.step((sched[rows, t] & live & ~forced).to(torch.int32))
        w = np.random.default_rng(8).standard_normal(K.N).astype(np.float32)
        for name, pol in _policies(ct, g).items():
            pol = dict(pol, require_budget=rb)
            out = A.imitation_gradient(pol, sched, env_weight=w, labels=labels)
            if name == "linear":
                ref = imitation_linear_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, pol["weight"], pol["bias"], g, E.G)
                got = np.concatenate([out["policy_gradient"]["weight"].double().cpu().numpy(),
                                      out["policy_gradient"]["bias"].double().cpu().numpy()[:, None]], axis=1)
                want = np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1)
                assert (np.abs(got - want) <= ref["bound"]).all(), (name, rb)
            else:
                ref = imitation_mlp_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, pol["layers"], pol["activation"], g, E.G)
                for (dW, db), (rW, rbias), (bW, bb) in zip(out["policy_gradient"]["layers"], ref["layers"], ref["bound"]):
                    assert (np.abs(dW.double().cpu().numpy() - rW) <= bW).all(), (name, rb)
                    assert (np.abs(db.double().cpu().numpy() - rbias) <= bb).all(), (name, rb)
            np.testing.assert_array_equal(out["days"].cpu().numpy(), ref["days"])
            assert (np.abs(out["log_likelihood"].double().cpu().numpy() - ref["ll"]) <= ref["ll_bound"]).all(), (name, rb)
        A.close()
        B.close()


def test_refusals_and_argument_checks(dev, tabs):
    from weather2alert_amd import HeatAlertVecEnv

    ct = tabs["mini"][0]
    env = HeatAlertVecEnv(64, tables=ct, device=dev, fixes={"lag"})
    env.reset(seed=1)
    sched = torch.zeros((64, ct.T), dtype=torch.bool, device=dev)
    with pytest.raises(ValueError, match="lag"):
        env.hindsight_values(sched)
    env.close()
    env = HeatAlertVecEnv(64, tables=ct, device=dev)
    env.reset(seed=1)
    for bad in (sched[:63], sched[:, :-1], sched.to(torch.int32), sched.float(), None):
        with pytest.raises(ValueError, match="alert_days"):
            env.hindsight_values(bad)
        with pytest.raises(ValueError, match="allowed_days"):
            env.hindsight_values(sched, allowed_days=sched[:63] if bad is None else bad)
    with pytest.raises(ValueError, match="n_steps"):
        env.hindsight_values(sched, n_steps=0)
    packed = env.hindsight_optimum()["alert_days"]
    from weather2alert_amd import policy as P
    words = P.pack_alert_days(packed, (ct.T + 31) // 32)
    _same(env.hindsight_values(packed), env.hindsight_values(words))
    part = env.hindsight_values(packed, n_steps=9)
    assert part["alert_gain"].shape == (9, 64) and set(part) == {"alert_gain", "expert_alert_days", "regret"}
    W = np.zeros((1, ct.n_obs), np.float32)
    pol = dict(kind="linear", weight=W, bias=np.zeros(1, np.float32))
    for bad in (sched[:63], sched.to(torch.int32)):
        with pytest.raises(ValueError, match="labels"):
            env.imitation_gradient(pol, sched, labels=bad)
    look = dict(pol, lookahead=dict(feature="heat_qi", days=3, weight=np.zeros((1, 3), np.float32)))
    with pytest.raises(ValueError, match="lookahead"):
        env.imitation_gradient(look, sched, labels=sched)
    # a start state outside the tables: NaN in the float outputs, no bits
    st = _clone(env.state())
    st["coef_col"][:5] = ct.S + 3
    st["finished"][5:9] = 1
    hv = env.hindsight_values(packed, start_state=st, value=True, loss=True)
    for f in FLOATS + ("regret",):
        x = hv[f] if f == "regret" else hv[f].T
        assert torch.isnan(x[:5]).all(), f
    assert torch.isnan(hv["alert_gain"][:, 5:9]).all() and (hv["value"][:, 5:9] == 0).all() and (hv["regret"][5:9] == 0).all()
    assert not hv["expert_alert_days"][:9].any() and env.check_status() == 0
    env.close()
