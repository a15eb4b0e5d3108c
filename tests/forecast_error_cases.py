"""The cases of tests/test_forecast_error_gpu.py, shared with tests/test_forecast_error_cpu.py, which walks every one of
them on the host oracle alone: the batch, groups, tables, reset settings and policies are those of
tests/lookahead_cases.py with the "error" and "error_seed" keys added. heat_qi is a quantile in [0, 1], so the MAE rows
are the reference's profile (2.5, 3.0, .., 7.0 for a feature in degrees) scaled to that range. Nothing here touches the
GPU or the library."""
import numpy as np

import forecast_error_restatement as FR
import lookahead_cases as C

N, G, GID0, SEED, FEATURE = C.N, C.G, C.GID0, C.SEED, C.FEATURE
ERROR_SCALAR = 0.125
ERROR_SCALE = 0.03  # row: 0.075, 0.09, .., 0.21
FEATURE_DAYS = (1, 3, 4, 5, 10)

# (table, D, sample, row): row = True takes the scaled profile, False the one scalar
LINEAR_CASES = [("mini", 1, False, False), ("mini", 3, True, True), ("ragged", 10, False, True),
                ("ragged", 4, True, False)]
# (net of policy_gradient_mlp_cases.MATRIX, D, sample): all six <WIDTH, LAYERS>; D = 4, 5, 10 are the k-step boundaries
# of the first layer's extra steps. D = 10 runs on the ragged table, the others on mini
MLP_CASES = [("tanh1_o2", 4, True), ("tanh7x13", 5, False), ("tanh17", 10, False), ("tanh29x9", 4, False),
             ("relu33", 10, True), ("relu40x64", 5, False), ("tanh64x33_o2", 10, True)]
GATE_CASES = [("linear", 3), ("mlp", 10)]  # on the ragged table
GATE_NET = C.GATE_NET
GRADIENT_CASES = [("mini", 3), ("ragged", 10)]  # sampled linear policies
IMITATION_CASES = [("mini", 3), ("ragged", 10)]
# error seeds moved off the default where a case met a near-tie on the host walk: case key -> seed
DEFAULT_ERROR_SEED = 11
ERROR_SEEDS = {}


def error_of(D, row=True):
    return [float(v) for v in FR.REFERENCE_MAE[:D] * np.float32(ERROR_SCALE)] if row else ERROR_SCALAR


def spec(D, row=True, key=None, **kw):
    return dict(C.spec(D), error=error_of(D, row), error_seed=ERROR_SEEDS.get(key, DEFAULT_ERROR_SEED), **kw)


def linear(ct, D, sample=False, row=True, key=None, **kw):
    return dict(C.linear(ct, D, sample, **kw), lookahead=spec(D, row, key))


def mlp(ct, name, D, sample=False, row=True, key=None, **kw):
    return dict(C.mlp(ct, name, D, sample, **kw), lookahead=spec(D, row, key))


def with_error(pol, error, **kw):
    """the policy with another "error" value (and, by keyword, another error_seed)"""
    return dict(pol, lookahead=dict(pol["lookahead"], error=error, **kw))


def without_error(pol):
    return dict(pol, lookahead=FR.clean(pol["lookahead"]))
