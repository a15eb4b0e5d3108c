"""The cases of tests/test_hindsight_values_{cpu,gpu}.py: N = 193 envs on the golden mini table and on the ragged table
of tests/table_edges.py, from reset and from a mid-episode state, Bernoulli schedules of attempts with p = 0.1 and 0.5
(attempts over budget occur), one env batch per budget as tests/test_hindsight_gpu.py::test_budget_cases arranges them:
0, 8 (at most (8 + 1)(8 + 4) / 2 = 54 states: one 64-state chunk), 40 (several chunks, in LDS) and 200 (the workspace
path on every env with more than 56 days left at T = 153). Nothing here touches the GPU at import."""
from __future__ import annotations

import os

import numpy as np

N = 193
TABLES = ("mini", "ragged")
BUDGETS = (0, 8, 40, 200)
STARTS = (0, 25)          # days stepped before the call
PS = (0.1, 0.5)           # the schedules' alert probability
CHUNKS = (7, 100)         # k of the chunking test: 7 changes a budget-40 env's U bin (alerts were issued), 100 leaves at
                          # most 53 days, whose DP fits in LDS whatever the budget (hs_day_bytes + hs_dp_bytes <= 64 KiB
                          # up to U = 56 at T = 153)
DAY_BAR = 1e-5            # the project's per-day reward bar of the f32 epilogue against fp64 (tests/test_env_gpu.py)
HS_KEYS = ("t", "used", "streak", "hist14", "budget", "n_days", "county_w", "year_i", "coef_col", "sample", "finished")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_tables():
    """name -> (compiled tables, env keywords)"""
    import table_edges as E
    from weather2alert_amd import tables

    return {"mini": (tables.CompiledTables.load_npz(os.path.join(GOLDEN, "mini_compiled.npz")), {}),
            "ragged": (E.make_tables()["ragged"].ct, dict(similar_climate_counties=True))}


def lds_fits(U, hb):
    """w2a_hindsight_optimum's split between LDS and the workspace (csrc/w2a_hindsight.hip.h)"""
    ns = (U + 1) * (U + 4) // 2
    return 32 * hb + 16 * ns + 8 * hb * ((ns + 63) // 64) <= 64 * 1024


def schedule(n, T, p, seed):
    return np.random.default_rng(seed).random((n, T)) < p


def prefix_actions(n, days, seed, p=0.5):
    return (np.random.default_rng(seed).random((days, n)) < p).astype(np.int32)
