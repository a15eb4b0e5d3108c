"""Observation layouts other than the generator's own (tests/test_obs_layouts_cpu.py, tests/test_obs_layouts_gpu.py).
tables._assign_slots derives the slot of every observation column from the column order and the weight key names of
the files it is given; every other table of the suite has the generator's order, whose layout is the identity on the
first 23 columns with every slot 0..28 taken. These four do not:

  permuted  the 21 exogenous columns in a seeded random order, the 7 endogenous columns reversed, two exogenous columns
            and `issued_in_advance` without coefficients: n_obs = 29, most columns on a slot that is not their index
  n28       permuted's exogenous order without `holiday`, endogenous columns in their own order, one exogenous column
            unweighted: n_obs = 28 (a multiple of 4), slot 28 empty
  n8        hi_max, heat_qi, dos + alert_lag1, alerts_2wks, alert_streak, remaining_budget, hi_max unweighted:
            n_obs = 8, heat_qi is column 1 on slot 0, run-time columns interleaved with a table column, slots 4..23 empty
  narrow    heat_qi + remaining_budget, alert_streak, alert_lag1: n_obs = 5, the smallest schema there is, the run-time
            slots in reverse order

and `permuted_ragged` / `n8_ragged`: the same schemas with episode lengths of 10..40 days, one pair at the full T and
the 1-, 2- and 3-day episodes of table_edges._lengths. Nothing here touches the GPU or the library's kernels."""
from __future__ import annotations

import copy

import numpy as np

import table_edges as E
from oracle import heatalert_oracle as O
from weather2alert_amd import synth

PERM_SEED = 7
BASE = dict(n_fips=30, years=[2006, 2007], n_days=40, n_samples=6, extra_confounder_fips=3, seed=41)
LAYOUTS = ("permuted", "n28", "n8", "narrow")
RAGGED = ("permuted_ragged", "n8_ragged")
N_OBS = {"permuted": 29, "n28": 28, "n8": 8, "narrow": 5, "permuted_ragged": 29, "n8_ragged": 8}
# reset settings in the style of table_edges.RESET, and env counts that are no multiple of 16 or 64
RESET = {name: dict(seed=50 + i, opts={"budget": 6}) for i, name in enumerate(LAYOUTS + RAGGED)}
N_ENVS, N_SMALL = 333, 70
# the seed of the sampled policies' uniforms: table_edges.POLICY_SEED unless a layout's references leave the near-tie cap
# with it (tests/test_obs_layouts_cpu.py: one of 70 envs of n28 under mlp16_sampled); the cap stays, the seed moves
POLICY_SEEDS = {"n28": 12}


def restrict(sd, exo_cols, endo_cols, unweighted=()):
    """A copy of `sd` with the exogenous columns `exo_cols` and the endogenous columns `endo_cols`, in the given order;
    columns that are gone and the columns of `unweighted` lose their baseline_* / effectiveness_* keys (both *_bias
    keys stay)."""
    out = copy.copy(sd)
    src = list(sd.meta["exo_cols"])
    out.exo = np.ascontiguousarray(sd.exo[..., [src.index(c) for c in exo_cols]])
    out.meta = dict(sd.meta, exo_cols=list(exo_cols), endo_cols=list(endo_cols))
    keep = (set(exo_cols) | set(endo_cols)) - set(unweighted) | {"bias"}
    out.weights = {k: v for k, v in sd.weights.items() if k.split("_", 1)[1] in keep}
    assert "baseline_bias" in out.weights and "effectiveness_bias" in out.weights
    return out


def permuted_exo():
    """synth.EXO_COLS in the order of one seeded permutation"""
    return [synth.EXO_COLS[i] for i in np.random.default_rng(PERM_SEED).permutation(len(synth.EXO_COLS))]


def schema(name):
    """(exogenous columns, endogenous columns, unweighted columns) of a layout"""
    px = permuted_exo()
    name = name.replace("_ragged", "")
    if name == "permuted":
        return px, synth.ENDO_COLS[::-1], (px[1], px[5], "issued_in_advance")
    if name == "n28":
        ex = [c for c in px if c != "holiday"]
        return ex, list(synth.ENDO_COLS), (ex[2],)
    if name == "n8":
        return ["hi_max", "heat_qi", "dos"], ["alert_lag1", "alerts_2wks", "alert_streak", "remaining_budget"], ("hi_max",)
    if name == "narrow":
        return ["heat_qi"], ["remaining_budget", "alert_streak", "alert_lag1"], ()
    raise KeyError(name)


def make_table(name):
    sd = restrict(synth.make_synth("linear", **BASE), *schema(name))
    nd = E._lengths(sd, 10, 40, 3) if name.endswith("_ragged") else None
    return E.Table(name, sd, nd)


def make_layouts(names=LAYOUTS + RAGGED):
    """name -> table_edges.Table"""
    return {name: make_table(name) for name in names}


def host_tuples(tb, n):
    return E.host_tuples(tb, n, RESET[tb.name])


def policy_seed(name):
    return POLICY_SEEDS.get(name, E.POLICY_SEED)


def make_policy(tb, pol_name, g):
    """table_edges.make_policy with the layout's policy seed"""
    pol, fn, ties = E.make_policy(tb.ct, pol_name, g)
    pol["seed"] = policy_seed(tb.name)
    return pol, fn, ties


def policy_uniform(tb, n):
    """the sampled policies' uniform of (env, episode 0, day t) under the layout's policy seed"""
    seed = policy_seed(tb.name)
    return lambda t: O.devrng_policy_uniform_vec(seed, E.GID0 + np.arange(n), np.zeros(n, np.int64), t)


def row32(ct, obs):
    """The kernels' row model: [..., n_obs] observation rows -> [..., 32] feature rows (zero in the other slots)"""
    out = np.zeros(obs.shape[:-1] + (32,), obs.dtype)
    out[..., np.asarray(ct.obs_slot)] = obs
    return out


def offset_column(ct):
    """a table-sourced observation column, not heat_qi, whose slot differs from its index (None when the layout has none)"""
    cands = [c for c, s in enumerate(ct.obs_slot[:-1]) if s != c and s < 24 and ct.columns[c] != "heat_qi"]
    # the one that varies most relative to its range (some columns of the generator are constant)
    def spread(c):
        x = ct.X[:, :, ct.obs_slot[c]]
        return float(x.std() / max(float(np.ptp(x)), 1e-9))
    return max(cands, key=spread) if cands else None
