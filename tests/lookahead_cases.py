"""The cases of tests/test_lookahead_gpu.py, shared with tests/test_lookahead_cpu.py, which walks every one of them on
the host oracle alone (the near-tie cap and "the policy decides" are properties of the seeds and the widened weights,
not of the kernels): batch size, groups, tables, reset settings, the policies and the case lists. Nothing here touches
the GPU or the library."""
import os
import types

import numpy as np

import lookahead_restatement as LR
import policy_gradient_mlp_cases as M
import table_edges as E
from oracle import heatalert_oracle as O
from weather2alert_amd import tables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, G, GID0, SEED = 193, 3, E.GID0, E.POLICY_SEED  # no multiple of 64; three groups
FEATURE = "heat_qi"
GATE_THRESHOLD = 0.6
MINI_RESET = dict(seed=5, opts={"budget": 10})

# (table, D, sample)
LINEAR_CASES = [("mini", 1, False), ("mini", 3, True), ("ragged", 10, False), ("ragged", 3, True)]
# (net of policy_gradient_mlp_cases.MATRIX, D, sample); D = 10 runs on the ragged table, the others on mini
MLP_CASES = [("tanh1_o2", 1, False), ("tanh7x13", 1, True), ("tanh17", 10, False), ("tanh29x9", 3, False),
             ("relu33", 10, True), ("relu40x64", 3, False), ("tanh64x33_o2", 10, True)]
# (kind, D), on the ragged table; the mlp case's net
GATE_CASES = [("linear", 3), ("mlp", 10)]
GATE_NET = "tanh17"
# (table, D): sampled linear policies whose group means must hold no near-tie env at all
GRADIENT_CASES = [("mini", 3), ("ragged", 10), ("mini", 1)]


def mlp_table(D):
    return "ragged" if D == 10 else "mini"


def make_tables():
    """name -> (compiled tables, reset settings, a callable giving a fresh host oracle)"""
    rg = E.make_tables()["ragged"]
    mini = tables.CompiledTables.load_npz(os.path.join(GOLDEN, "mini_compiled.npz"))
    mini_root = os.path.join(GOLDEN, "mini")
    return {"mini": (mini, MINI_RESET, lambda: O.VectorOracle(O.RefData.from_files(mini_root, weights="linear", split="65k"),
                                                              mini.fips_weather, mini.years)),
            "ragged": (rg.ct, E.RESET["ragged"], rg.oracle)}


def host_tuples(name, tb):
    """the episode tuples env.reset(seed, options) draws for the N envs of the GPU tests (table_edges.host_tuples)"""
    return E.host_tuples(types.SimpleNamespace(ct=tb[0], name=name), N, tb[1])


def groups():
    return (np.arange(N) * 3 + np.arange(N) // 7) % G


def spec(D):
    return {"feature": FEATURE, "days": D}


def linear(ct, D, sample=False, seed=3, **kw):
    W, b = E.linear_params(ct, seed=seed)
    W = LR.widen_linear(ct, W[:G], D, seed=seed + D)
    return dict(kind="linear", weight=W, bias=b[:G], group=groups(), sample=sample, seed=SEED, lookahead=spec(D), **kw)


def mlp(ct, name, D, sample=False, **kw):
    _, hidden, act, n_out = M.MATRIX[name]
    layers = [(W[:G], b[:G]) for W, b in LR.widen_net(M.net(ct, name, hidden, n_out), D, seed=D + len(name))]
    return dict(kind="mlp", layers=layers, activation=act, group=groups(), sample=sample, seed=SEED,
                lookahead=spec(D), **kw)


def logit_fn(pol):
    """x = cat(obs, f) -> (fp64 logit, near-tie scale), as the reference tests evaluate their policies"""
    if pol["kind"] == "linear":
        return lambda x: LR.linear_logit(pol["weight"], pol["bias"], pol["group"], x)
    return lambda x: E.mlp64(pol["layers"], pol["activation"], x, pol["group"])
